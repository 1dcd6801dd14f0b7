"""The list of k_search4 instantiations (fmx_search4.h, FMX_SEARCH4_LIST) against the recipe table (tests/search_forms.py):
an instantiation added without a recipe fails here, and so does a recipe for a form that no longer exists.  The batteries
the GPU tests search are checked here too, on the oracle alone: enough hits, enough misses, a miss in every region."""
import numpy as np
import pytest

import oracle
import search_forms as sf
from helpers import pack_patterns


def test_recipes_are_the_headers_list(tmp_path):
    forms = sf.header_forms(tmp_path)
    assert len(forms) == len(set(forms)), "FMX_SEARCH4_LIST names a form twice: %s" % sorted(f for f in set(forms) if forms.count(f) > 1)
    missing = sorted(set(forms) - set(sf.RECIPES))
    stale = sorted(set(sf.RECIPES) - set(forms))
    assert not missing, "instantiations without a recipe: " + ", ".join(sf.form_str(f) for f in missing)
    assert not stale, "recipes for forms that FMX_SEARCH4_LIST does not hold: " + ", ".join(sf.form_str(f) for f in stale)
    assert len(forms) == 90      # 64 one-hot, 20 bytes-layout, 6 with level K+1


def test_every_recipe_belongs_to_one_group_a_gpu_test_runs():
    ids = [r["id"] for rs in sf.RECIPES.values() for r in rs]
    assert len(ids) == len(set(ids))
    run = [r["id"] for g in sf.SMALL_GROUPS + sf.WIDE_GROUPS for r in sf.recipes_of(g)]
    assert sorted(run) == sorted(ids)
    for f, rs in sf.RECIPES.items():
        for r in rs:
            assert r["form"] == f and (r["index"]["kind"] == "wide") == bool(f[0] and f[1] == sf.ONEHOT)
            # the pool serves the forms with pairs of lanes or a row table walked by single lanes: their many-batches run must draw from it
            assert r["pool"] == bool(f[6] or f[4])


def test_small_recipes_name_the_depth_the_rule_gives():
    for rs in sf.RECIPES.values():
        for r in rs:
            spec = r["index"]
            if spec["kind"] == "iid":
                k = sf.ktab_rule(spec["n"], spec["sigma"]) if r["keys"]["ktab"] == "auto" else 0
                assert sf.kt_of(k) == r["form"][2], r["id"]
            elif spec["kind"] == "wide":
                assert sf.ktab_rule(spec["n"], spec["sigma"]) == 14 and spec["n"] > 1 << 32
                assert (spec["n"] - (1 << 32)) * 9 >= spec["n"] * 0.99      # a ninth of the rows lie above 2^32


@pytest.mark.parametrize("group", sf.SMALL_GROUPS)
def test_battery_conditions_hold_on_the_oracle(group):
    seen = {}
    for r in sf.recipes_of(group):
        key = (str(r["index"]), r["form"][2])
        if key not in seen:
            bwt, eof, counts = sf.small_index(r["index"])
            orc = oracle.NaiveFMSearcher.from_mem(bwt, eof, counts)
            syms = [int(s) for s in np.nonzero(counts)[0] if s != 0]
            if r["index"]["kind"] == "rep":
                assert sf.kt_of(sf.ktab_rule(orc.n, len(syms))) == 4
            buf, off = pack_patterns(sf.battery(orc, syms, r["form"][2], sf.JUMP_CHARS, 7 + r["form"][2], ragged=1500))
            seen[key] = (orc, buf, off, orc.search_batch(buf, off))
        orc, buf, off, out = seen[key]
        fig = sf.check_conditions(r["form"], orc, buf, off, *out)
        assert fig["patterns"] > 3000
