"""Every instantiation of k_search4 is launched and held to an oracle (tests/search_forms.py has the recipes; the CPU test
test_search_forms_cpu.py holds them to FMX_SEARCH4_LIST).  FMX_TRACE is read once per process, so every group of recipes runs
in a child process, one at a time; the parent attributes the launch lines on the child's stderr to the recipe whose markers
enclose them and fails a recipe whose handle chose another form.  Needs a real MI355X:  pytest -m gpu -s

  * test_small_forms: the 58 forms up to 2^32 rows and of the bytes layout on indexes of about 2^16 rows (and one repetitive
    text per layout), against oracle.NaiveFMSearcher: intervals bit for bit, misses' values and executed steps included, the
    8-byte form and FMX_SEARCH_MISS_NONE.  Its battery of edges is a few thousand patterns: ONE batch per wave (launch_form
    spreads a batch over as many workgroups as it has batches for);
  * test_small_forms_pool: the same 58 forms and the same comparisons with FMX_SEARCH_WGS=1 (1024 waves) over 4608
    batches, so that every form's batch loop goes round -- the next batch staged while one is searched, parked misses walked
    and the rows phase run inside the loop -- and the forms that can draw their last rounds from the pool do;
  * test_wide_forms: the 32 one-hot forms above 2^32 rows on one index of 2^32 + 2^29 + 12345 rows, against
    oracle.SampledFMSearcher over the same bytes -- an independent reference, not the product's own getPrevRange; also with
    FMX_SEARCH_WGS=1, four or nine batches per wave.
The parent reads "N batches over M waves" from the launch lines and fails a recipe of the last two tests that had no launch
with N >= 3 M.

A child that does not end with status 0 and its last line -- a signal, an abort, its time limit, or an error of the library
that the child did not expect -- fails its test and every later test of this module at once: nothing is started on a device
that may just have faulted, and nothing is retried.
"""
import gc
import json
import os
import re
import subprocess
import sys

import pytest

import search_forms as sf

pytestmark = pytest.mark.gpu

_FAULT = []      # why no further child is started
# Seconds for one child ("Which instantiation a search launches").  Above 2^32 rows: three times the 16.9-19.7 s
# a child took on the MI355X.  The small children took 2.3-7.6 s, alone and inside the whole suite: 30 s is three times the
# slowest and more than that for the others -- most of a small child's time is the start of the interpreter, the library and
# the device, which follows the machine's load and not the work, so the bound is not taken lower.
SMALL_TIMEOUT = 30
MANY_TIMEOUT = 30
WIDE_TIMEOUT = 60

_LAUNCH = re.compile(r"^\[fmx\] (k_search4<[\d,]+>)( census)?:(.*)$")
_DRAWN = re.compile(r"the last (\d+) drawn from ticket area (\d+)")
_ROUNDS = re.compile(r"(\d+) batches over (\d+) waves")


def run_child(mode, group, timeout, env_extra):
    """One child, alone on the device; returns (its recipes, their results by recipe id, their k_search4 trace lines by recipe id)."""
    if _FAULT:
        pytest.fail("not started: " + _FAULT[0])
    recipes = sf.recipes_of(group)
    env = dict(os.environ, FMX_TRACE="1", **env_extra)
    for r in recipes:
        env.update(r["env"])
        assert r["env"] == recipes[0]["env"], "one process environment per group"
    try:
        p = subprocess.run([sys.executable, os.path.join(sf.TESTS, "search_forms.py"), mode, group], capture_output=True, text=True,
                           timeout=timeout, env=env)
    except subprocess.TimeoutExpired as e:
        _FAULT.append("the child of %s %s did not end within %d s" % (mode, group, timeout))
        pytest.fail(_FAULT[0] + "\n" + str(e.stderr)[-2000:])
    if p.returncode != 0 or not p.stdout.rstrip().endswith("DONE"):
        # (a recipe that disagrees with its oracle is reported in the child's results and does not end the child)
        _FAULT.append("the child of %s %s ended with status %d%s" % (mode, group, p.returncode, "" if p.returncode else " before its last line"))
        pytest.fail(_FAULT[0] + "\n" + p.stdout[-1500:] + p.stderr[-3000:])
    results = {}
    for ln in p.stdout.splitlines():
        if ln.startswith("RESULT "):
            r = json.loads(ln[7:])
            results[r["id"]] = r
    trace, cur = {}, None
    for ln in p.stderr.splitlines():
        if ln.startswith("[forms] begin "):
            cur = ln.split()[2]
            trace[cur] = []
        elif ln.startswith("[forms] end "):
            cur = None
        else:
            m = _LAUNCH.match(ln)
            if m:
                assert cur is not None, "a launch outside every recipe's markers: " + ln
                trace[cur].append((m.group(1), bool(m.group(2)), m.group(3)))
    return recipes, results, trace


def check_recipes(recipes, results, trace, many=False):
    """Per recipe: the child's comparison passed, every launch between its markers names exactly its form (a census line its
    form or the twin by the other lane grouping), and there was at least one launch.  many: every launch had MIN_ROUNDS
    batches per wave or more, and where the form can draw its last rounds from the pool, a launch did."""
    failures, seen = [], set()
    for r in recipes:
        rid, name = r["id"], sf.form_str(r["form"])
        res = results.get(rid)
        lines = trace.get(rid, [])
        launches = [n for n, census, _ in lines if not census]
        print("%-48s %-32s %3d launches  %s" % (rid, name, len(launches), json.dumps(res.get("figures", {})) + " %.1f s" % res.get("seconds", 0) if res else "no result"))
        if res is None:
            failures.append("%s: the child reported nothing" % rid)
            continue
        other = sorted({n for n in launches if n != name})
        census = sorted({n for n, c, _ in lines if c and n not in (name, sf.form_str(sf.twin(r["form"])))})
        if other or not launches:
            failures.append("%s: wants %s, launched %s" % (rid, name, other or "nothing"))
        else:
            seen.add(r["form"])
        if census:
            failures.append("%s: wants %s, calibrated %s" % (rid, name, census))
        if not res["ok"]:
            failures.append("%s (%s): %s" % (rid, name, res.get("error")))
        rests = [rest for _, c, rest in lines if not c]
        rounds = [(int(m.group(1)), int(m.group(2))) for m in map(_ROUNDS.search, rests) if m]
        if many and (len(rounds) != len(rests) or not rounds or any(nb < sf.MIN_ROUNDS * nw for nb, nw in rounds)):
            failures.append("%s (%s): a launch with fewer than %d batches per wave: %s" % (rid, name, sf.MIN_ROUNDS, rests[:3]))
        if many and r["pool"] and not any(int(m.group(1)) > 0 and int(m.group(2)) > 0 for m in map(_DRAWN.search, rests) if m):
            failures.append("%s (%s): no launch drew its last rounds from the pool: %s" % (rid, name, rests[:3]))
    assert not failures, "\n".join(failures)
    return seen


@pytest.mark.timeout(SMALL_TIMEOUT + 60)
@pytest.mark.parametrize("group", sf.SMALL_GROUPS)
def test_small_forms(group):
    recipes, results, trace = run_child("small", group, SMALL_TIMEOUT, {})
    seen = check_recipes(recipes, results, trace)
    assert seen == {r["form"] for r in recipes}
    print("%s: %d forms launched and equal to the oracle: %s" % (group, len(seen), " ".join(sf.form_str(f) for f in sorted(seen))))


@pytest.mark.timeout(MANY_TIMEOUT + 60)
@pytest.mark.parametrize("group", sf.SMALL_GROUPS)
def test_small_forms_pool(group):
    """Many batches per wave for EVERY form, and the pool's last rounds for the forms that have one (see the module's text)."""
    recipes, results, trace = run_child("many", group, MANY_TIMEOUT, {"FMX_SEARCH_WGS": "1"})
    seen = check_recipes(recipes, results, trace, many=True)
    assert seen == {r["form"] for r in recipes}


@pytest.mark.timeout(WIDE_TIMEOUT + 60)
@pytest.mark.parametrize("group", sf.WIDE_GROUPS)
def test_wide_forms(group):
    """Per form 147 456 patterns (LF walks of the device, a third with one byte replaced inside the alphabet, lengths 1 .. 40, and
    every pattern of one and two characters): sp, ep and executed steps equal to the reference's.  On the reference's outputs:
    at least 5 % of the hits have sp >= 2^32, at least one interval has sp < 2^32 <= ep, at least 1000 misses end at a row
    >= 2^32 (the child asserts them per form; the figures are printed here)."""
    try:
        import torch
        gc.collect()
        torch.cuda.empty_cache()      # the child needs about 190 GiB: nothing this process caches may stay
    except ImportError:
        pass
    recipes, results, trace = run_child("wide", group, WIDE_TIMEOUT, {"FMX_SEARCH_WGS": "1"})
    setup = results.get(group)
    assert setup is not None and setup["ok"], setup
    print(group, json.dumps(setup["figures"]))
    seen = check_recipes(recipes, results, trace, many=True)
    assert seen == {r["form"] for r in recipes} and len(seen) == 8
    assert all(f[0] == 1 and f[1] == sf.ONEHOT for f in seen)
