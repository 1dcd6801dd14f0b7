"""Approximate search without a device: the two expectations of tests/approx_ref.py against each other, the layout of
the two new structs against a strict-C compile of the header, and every refusal fmx_search_approx_batch decides on the
host."""
import ctypes
import itertools
import os
import shutil
import subprocess

import numpy as np
import pytest

import approx_ref
from conftest import ROOT
from findex_amd import _lib

ARG, OVERFLOW = 3, 9


def test_the_two_references_agree_on_tiny_inputs():
    rng = np.random.default_rng(7)
    s = bytes(rng.integers(97, 100, 60, dtype=np.uint8))          # sigma = 3
    orc = approx_ref.index_of(s)[0]
    hits = 0
    for m in range(1, 5):
        for P in itertools.product(b"abc", repeat=m):
            P = bytes(P)
            for e in range(4):
                w = approx_ref.window_hits(s, P, e)
                assert w == approx_ref.dfs_hits(orc, P, e), (P, e)
                assert w == approx_ref.within(approx_ref.window_hits(s, P, 3), e), (P, e)
                hits += len(w)
            # a range that leaves out one letter of the text, and one that leaves out all
            assert approx_ref.window_hits(s, P, 2, 98, 99) == approx_ref.dfs_hits(orc, P, 2, 98, 99), P
            assert approx_ref.window_hits(s, P, 3, 1, 96) == approx_ref.dfs_hits(orc, P, 0), P
    assert hits > 5000
    ends = 0
    for m in range(1, 4):                                        # byte 0 in a pattern: only the sentinel behind the text holds it
        for P in itertools.product(b"ab\0", repeat=m):
            for e in range(3):
                w = approx_ref.window_hits(s, bytes(P), e)
                assert w == approx_ref.dfs_hits(orc, bytes(P), e), (P, e)
                ends += len(w) if 0 in P else 0
    assert ends > 20
    assert approx_ref.window_hits(s, b"", 2) == approx_ref.dfs_hits(orc, b"", 2) == [(0, 61, 0)]


def test_the_restated_walk_against_both_references_and_the_oracles_steps():
    """approx_ref.walk on the same tiny inputs: its hits are dfs_hits' (which has no one-row shortcut and no candidate
    list), for the ranges that leave letters out and for byte 0 as well; at e = 0 its steps are the oracle's search_batch
    steps; and its steps obey what the description fixes without any kernel: a larger budget never makes fewer steps, and a
    range without a letter of the index makes exactly the steps of e = 0."""
    from helpers import pack_patterns
    rng = np.random.default_rng(7)
    s = bytes(rng.integers(97, 100, 60, dtype=np.uint8))
    orc = approx_ref.index_of(s)[0]
    pats = [bytes(P) for m in range(1, 5) for P in itertools.product(b"abc", repeat=m)]
    pats += [bytes(P) for m in range(1, 4) for P in itertools.product(b"ab\0", repeat=m)]
    pats += [b"", s[:12], s[20:44], s[-9:], s, s + b"a", b"z" + s[3:9], s[3:9] + b"z"]
    buf, off = pack_patterns(pats)
    _, _, exact = orc.search_batch(buf, off)
    one_row = 0
    for P, st0 in zip(pats, exact.tolist()):
        before = None
        for e in range(4):
            hits, steps = approx_ref.walk(orc, P, e)
            assert hits == approx_ref.dfs_hits(orc, P, e), (P, e)
            assert before is None or steps >= before, (P, e)
            before = steps
            if e == 0:
                assert steps == st0, (P, steps, st0)
            one_row += sum(1 for sp, ep, d in hits if ep - sp == 1 and d == e)
        for sub in ((98, 99), (97, 97), (99, 255)):
            assert approx_ref.walk(orc, P, 2, *sub)[0] == approx_ref.dfs_hits(orc, P, 2, *sub), (P, sub)
        hits, steps = approx_ref.walk(orc, P, 3, 1, 96)
        assert hits == approx_ref.dfs_hits(orc, P, 0) and steps == st0, P
    assert one_row > 500                                     # hits that were reached through nodes of one row
    assert approx_ref.walk(orc, b"", 2) == ([(0, 61, 0)], 0)
    # the step count by hand: sigma = 3, one pattern byte, e = 1: two candidates and the match step
    assert approx_ref.walk(orc, b"a", 1)[1] == 3 and approx_ref.walk(orc, b"a", 1, 98, 99)[1] == 3
    assert approx_ref.walk(orc, b"z", 1)[1] == 4 and approx_ref.walk(orc, b"a", 1, 97, 97)[1] == 1


def test_the_restated_walk_on_a_synthetic_bwt_and_the_sampled_searcher():
    """A BWT that is no text's (the EOF slot first, in the middle, last), and oracle.SampledFMSearcher, which has no
    bwt_read: the row's symbol comes from occ there.  Both searchers give the same hits and the same steps."""
    import oracle
    from helpers import lf_walk_patterns, synth_bwt
    for eof in (0, 150, 299):
        index = synth_bwt(300, 97, 100, seed=9, eof=eof)
        orc = oracle.NaiveFMSearcher.from_mem(*index)
        smp = oracle.SampledFMSearcher(index[0], eof)
        rng = np.random.default_rng(eof)
        pats = lf_walk_patterns(orc, rng, 30, 7, 0.5, alphabet=[97, 98, 99, 100])
        for r in range(0, 300, 37):
            assert approx_ref.row_symbol(smp, r) == approx_ref.row_symbol(orc, r) == (0 if r == eof else int(index[0][r]))
        assert approx_ref.row_symbol(smp, eof) == 0
        for P in pats:
            for e in range(3):
                got = approx_ref.walk(orc, P, e)
                assert got[0] == approx_ref.dfs_hits(orc, P, e), (eof, P, e)
                assert approx_ref.walk(smp, P, e) == got, (eof, P, e)
        smp.close()


def test_struct_layouts():
    assert ctypes.sizeof(_lib.fmx_approx_hit) == 24
    assert ctypes.sizeof(_lib.fmx_approx_opts) == 8
    assert _lib.fmx_approx_hit.sp.offset == 8 and _lib.fmx_approx_hit.ep.offset == 16
    assert _lib.fmx_approx_opts.sub_lo.offset == 4 and _lib.fmx_approx_opts.sub_hi.offset == 5
    assert _lib.fmx_approx_opts.reserved.offset == 6


@pytest.mark.skipif(shutil.which("gcc") is None, reason="needs gcc")
def test_struct_layouts_against_a_strict_c_compile(tmp_path):
    src = tmp_path / "sizes.c"
    src.write_text(
        "#include <stddef.h>\n#include <stdio.h>\n#include <fmx.h>\n"
        "int main(void) {\n"
        "  printf(\"%d %d %d %d %d %d\\n\", (int)sizeof(fmx_approx_hit), (int)sizeof(fmx_approx_opts),\n"
        "         (int)offsetof(fmx_approx_hit, sp), (int)offsetof(fmx_approx_opts, sub_hi),\n"
        "         (int)offsetof(fmx_approx_opts, reserved), FMX_APPROX_MAX_MISMATCHES);\n"
        "  return 0;\n}\n")
    exe = tmp_path / "sizes"
    subprocess.check_call(["gcc", "-std=c99", "-Wall", "-Wextra", "-Werror", "-pedantic", "-I" + os.path.join(ROOT, "include"),
                           str(src), "-o", str(exe)])
    out = subprocess.run([str(exe)], capture_output=True, text=True, timeout=60)
    assert out.stdout.split() == ["24", "8", "8", "5", "6", "3"]


def test_abi_version_and_stats_size_stay():
    assert _lib.load().fmx_abi_version() == 5
    assert ctypes.sizeof(_lib.fmx_stats_t) == 232


def test_argument_refusals_before_any_device():
    """Everything the call decides from its arguments alone comes before the handle is looked at, and the null handle is
    refused last with a message of its own: on a machine without a GPU, where no handle can be opened, each refusal still
    shows by its message.  What needs a real handle -- FMX_ERR_UNSUPPORTED for fmx_open_block -- is in
    tests/test_gpu_approx.py."""
    L = _lib.load()
    n_out = ctypes.c_size_t(77)
    pat = np.frombuffer(b"abcd", dtype=np.uint8)
    off = np.array([0, 2, 4], dtype=np.uint64)
    out_off = np.zeros(3, dtype=np.uint64)
    out = np.zeros(4, dtype=[("pattern", np.uint32), ("mismatches", np.uint32), ("sp", np.uint64), ("ep", np.uint64)])

    def host(h=None, o=off, k=2, opts=None, cap=4, n=n_out, oo=out_off):
        return L.fmx_search_approx_batch(h, pat.ctypes.data, o.ctypes.data, k, ctypes.byref(opts) if opts is not None else None,
                                         oo.ctypes.data if oo is not None else None, out.ctypes.data, cap,
                                         ctypes.byref(n) if n is not None else None)

    def dev(h=None, k=2, opts=None, cap=4, n=n_out):
        return L.fmx_search_approx_batch_dev(h, pat.ctypes.data, off.ctypes.data, k, ctypes.byref(opts) if opts is not None else None,
                                             out_off.ctypes.data, out.ctypes.data, cap, ctypes.byref(n) if n is not None else None, None)

    O = _lib.fmx_approx_opts
    cases = [
        (dict(), b"handle"),
        (dict(n=None), b"n_out"),
        (dict(opts=O(4, 0, 0, 0)), b"max_mismatches"),
        (dict(opts=O(2 ** 32 - 1, 0, 0, 0)), b"max_mismatches"),
        (dict(opts=O(1, 5, 4, 0)), b"sub_lo > sub_hi"),
        (dict(opts=O(1, 0, 9, 0)), b"symbol 0"),
        (dict(opts=O(1, 9, 0, 0)), b"symbol 0"),
        (dict(opts=O(1, 1, 255, 1)), b"reserved"),
        (dict(k=(1 << 26) + 1), b"2^26"),
        (dict(cap=1 << 32), b"2^32"),
    ]
    for form in (host, dev):
        for kw, word in cases:
            assert form(**kw) == ARG, (form.__name__, kw)
            assert word in L.fmx_last_error(), (form.__name__, kw, L.fmx_last_error())
    assert host(o=np.array([0, 3, 2], dtype=np.uint64)) == ARG and b"non-decreasing" in L.fmx_last_error()
    assert host(oo=None) == ARG and b"null argument" in L.fmx_last_error()
    assert n_out.value == 77                                 # a refused call writes nothing
    a, b = ctypes.c_double(-1), ctypes.c_double(-1)
    c, d = ctypes.c_uint64(5), ctypes.c_uint64(5)
    assert L.fmx_approx_last(ctypes.byref(a), ctypes.byref(b), ctypes.byref(c), ctypes.byref(d)) == 0
    assert a.value >= 0 and b.value >= 0
    assert L.fmx_approx_last(None, None, None, None) == 0
