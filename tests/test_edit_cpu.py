"""Edit-distance search without a device (fmx_search_edit_batch): the three expectations of tests/edit_ref.py
against each other on random small cases, hand-worked cases, the e = 0 steps against the oracle's exact search, the layout
of the two structs against a strict-C compile of the header, and every refusal the calls decide on the host.  What needs a
handle -- FMX_ERR_UNSUPPORTED for fmx_open_block, the device form's long pattern -- is in tests/test_gpu_edit.py: no handle
opens without a device."""
import ctypes
import os
import shutil
import subprocess

import numpy as np
import pytest

import approx_ref
import edit_ref
from conftest import ROOT
from findex_amd import _lib
from helpers import pack_patterns

ARG = 3
RANGES = ((1, 255), (98, 255), (97, 98), (99, 255), (1, 96))


def test_the_three_references_agree_on_random_small_cases():
    """Texts of 1 .. 40 bytes over 2 .. 4 letters, patterns of 0 .. 8 bytes (half of them taken from the text, with a letter
    the text may lack among the others), e = 0 .. 2, ranges that leave letters out."""
    rng = np.random.default_rng(3)
    cases = hits = edits = 0
    for _ in range(700):
        sigma = int(rng.integers(2, 5))
        s = bytes(rng.integers(97, 97 + sigma, int(rng.integers(1, 41)), dtype=np.uint8))
        orc = approx_ref.index_of(s)[0]
        for _ in range(3):
            m = int(rng.integers(0, 9))
            P = bytes(rng.integers(97, 97 + sigma + 1, m, dtype=np.uint8))
            if rng.random() < 0.5 and 0 < m < len(s):
                at = int(rng.integers(0, len(s) - m))
                P = s[at:at + m]
            e = int(rng.integers(0, 3))
            lo, hi = RANGES[int(rng.integers(0, len(RANGES)))]
            b = edit_ref.brute_hits(s, P, e, lo, hi)
            assert b == edit_ref.dfs_hits(orc, P, e, lo, hi), (s, P, e, lo, hi)
            assert b == edit_ref.walk(orc, P, e, lo, hi)[0], (s, P, e, lo, hi)
            cases += 1
            hits += len(b)
            edits += sum(1 for h in b if h[3] == 2)
    print("random cases: %d, hits %d, of them with d = 2: %d" % (cases, hits, edits))
    assert cases >= 2000 and hits > 5_000 and edits > 1_000


def test_a_pattern_with_byte_zero_dfs_against_walk():
    """Only the sentinel behind the text holds byte 0, and the reference's loop steps over it: dfs_hits and walk rest on
    getPrevRange alone and must agree there too."""
    rng = np.random.default_rng(4)
    found = 0
    for _ in range(60):
        s = bytes(rng.integers(97, 100, int(rng.integers(3, 30)), dtype=np.uint8))
        orc = approx_ref.index_of(s)[0]
        for P in (b"\0", s[-2:] + b"\0", b"\0" + s[:2], s[-1:] + b"\0" + s[:1], b"a\0b", b"\0\0"):
            for e in range(3):
                d = edit_ref.dfs_hits(orc, P, e)
                assert d == edit_ref.walk(orc, P, e)[0], (s, P, e)
                found += len(d)
    assert found > 1000


def test_hand_worked_cases():
    def hits(s, P, e, **kw):
        got = edit_ref.brute_hits(s, P, e, **kw)
        orc = approx_ref.index_of(s)[0]
        assert got == edit_ref.dfs_hits(orc, P, e, **kw) == edit_ref.walk(orc, P, e, **kw)[0]
        return {(s_[0], s_[1], s_[3]) for s_ in got}, orc

    def row(orc, Q, d):
        return (orc.search(Q)[0], len(Q), d)

    # abc in abxc: x inserted (abxc), c deleted (ab), c replaced (abx); bxc and xc are two edits away
    got, orc = hits(b"abxc", b"abc", 1)
    assert got == {row(orc, b"abxc", 1), row(orc, b"ab", 1), row(orc, b"abx", 1)}
    got2, _ = hits(b"abxc", b"abc", 2)
    assert got < got2 and {row(orc, b"bxc", 2), row(orc, b"xc", 2), row(orc, b"a", 2)} <= got2
    # abc in ac: the b deleted
    got, orc = hits(b"ac", b"abc", 1)
    assert got == {row(orc, b"ac", 1)}
    # abc in abcc: exact, and one c inserted; bc and ab by a deletion
    got, orc = hits(b"abcc", b"abc", 1)
    assert got == {row(orc, b"abc", 0), row(orc, b"abcc", 1), row(orc, b"ab", 1), row(orc, b"bc", 1)}
    assert row(orc, b"bcc", 2) in hits(b"abcc", b"abc", 2)[0]
    # m <= e: the empty string is a hit with d = m, the interval (0, n)
    got, orc = hits(b"abab", b"ab", 2)
    assert (0, 0, 2) in got and row(orc, b"ab", 0) in got and row(orc, b"abab", 2) in got
    assert edit_ref.walk(orc, b"ab", 2)[0][0] == (0, 0, orc.n, 2)
    got, _ = hits(b"abab", b"ab", 1)
    assert all(ln > 0 for _, ln, _ in got)
    # the empty pattern: (0, n) with d = 0 and every occurring string over the range of 1 .. e bytes
    got, orc = hits(b"abca", b"", 2)
    assert got == {(0, 0, 0)} | {row(orc, Q, len(Q)) for Q in (b"a", b"b", b"c", b"ab", b"bc", b"ca")}
    got, orc = hits(b"abca", b"", 2, lo=98, hi=99)
    assert got == {(0, 0, 0), row(orc, b"b", 1), row(orc, b"c", 1), row(orc, b"bc", 2)}
    assert hits(b"abca", b"", 0)[0] == {(0, 0, 0)}
    # a hit whose only alignment uses one insertion and one deletion: abcd -> bcdx (a deleted, x inserted), same length
    got, orc = hits(b"zbcdxz", b"abcd", 2)
    assert row(orc, b"bcdx", 2) in got and row(orc, b"bcd", 1) in got
    assert sum(1 for x, y in zip(b"bcdx", b"abcd") if x != y) == 4           # four substitutions otherwise
    # a byte outside the range is neither inserted nor substituted, but it may be deleted and it matches itself
    got, orc = hits(b"abxc", b"abc", 1, lo=97, hi=99)
    assert got == {row(orc, b"ab", 1)}
    got, orc = hits(b"abxc", b"abxc", 1, lo=97, hi=99)
    assert row(orc, b"abxc", 0) in got and row(orc, b"abx", 1) in got and row(orc, b"bxc", 1) in got


def test_budget_zero_makes_the_steps_of_the_exact_search():
    rng = np.random.default_rng(7)
    s = bytes(rng.integers(97, 100, 60, dtype=np.uint8))
    orc = approx_ref.index_of(s)[0]
    pats = [b"", s[:12], s[20:44], s[-9:], s, s + b"a", b"z" + s[3:9], s[3:9] + b"z", b"abc\0", b"\0ab"]
    pats += [bytes(rng.integers(97, 100, int(rng.integers(1, 6)), dtype=np.uint8)) for _ in range(100)]
    pats += [bytes(rng.integers(97, 101, int(rng.integers(1, 9)), dtype=np.uint8)) for _ in range(100)]
    buf, off = pack_patterns(pats)
    sp, ep, exact = orc.search_batch(buf, off)
    missed = 0
    for P, a, b, st0 in zip(pats, sp.tolist(), ep.tolist(), exact.tolist()):
        hits, steps = edit_ref.walk(orc, P, 0)
        assert steps == st0, (P, steps, st0)
        assert hits == ([(a, len(P), b, 0)] if a < b else []), P
        missed += a >= b
        before = steps
        for e in (1, 2):                                     # a larger budget never makes fewer steps
            more = edit_ref.walk(orc, P, e)[1]
            assert more >= before, (P, e)
            before = more
        assert edit_ref.walk(orc, P, 2, 1, 96)[0] == edit_ref.dfs_hits(orc, P, 2, 1, 96), P      # deletions only
    assert 50 < missed < len(pats) - 50                      # misses that end on several rows, and on one
    # the step count by hand: sigma = 3, one pattern byte.  e = 1: the root has budget -- three candidates (the pattern's byte is
    # one of them); the children a, b, c have min R = 0, 1, 1: a steps its three candidates again, b and c have M = {a}
    assert edit_ref.walk(orc, b"a", 0)[1] == 1
    assert edit_ref.walk(orc, b"a", 1)[1] == 3 + 3 + 1 + 1
    assert edit_ref.walk(orc, b"z", 1)[1] == 3 + 1 + 3 * 1      # z is tried too, comes back empty; a, b, c have M = {z}


def test_struct_layouts():
    assert ctypes.sizeof(_lib.fmx_edit_hit) == 24
    assert ctypes.sizeof(_lib.fmx_edit_opts) == 8
    assert _lib.fmx_edit_hit.edits.offset == 4 and _lib.fmx_edit_hit.len.offset == 6
    assert _lib.fmx_edit_hit.sp.offset == 8 and _lib.fmx_edit_hit.ep.offset == 16
    assert _lib.fmx_edit_opts.sub_lo.offset == 4 and _lib.fmx_edit_opts.sub_hi.offset == 5
    assert _lib.fmx_edit_opts.reserved.offset == 6
    import findex_amd
    assert findex_amd.HipFMSearcher.EDIT_HIT.itemsize == 24
    assert [findex_amd.HipFMSearcher.EDIT_HIT.fields[f][1] for f in ("pattern", "edits", "len", "sp", "ep")] == [0, 4, 6, 8, 16]


@pytest.mark.skipif(shutil.which("gcc") is None, reason="needs gcc")
def test_struct_layouts_against_a_strict_c_compile(tmp_path):
    src = tmp_path / "sizes.c"
    src.write_text(
        "#include <stddef.h>\n#include <stdio.h>\n#include <fmx.h>\n"
        "int main(void) {\n"
        "  printf(\"%d %d %d %d %d %d %d %d %d\\n\", (int)sizeof(fmx_edit_hit), (int)sizeof(fmx_edit_opts),\n"
        "         (int)offsetof(fmx_edit_hit, edits), (int)offsetof(fmx_edit_hit, len), (int)offsetof(fmx_edit_hit, sp),\n"
        "         (int)offsetof(fmx_edit_opts, sub_hi), (int)offsetof(fmx_edit_opts, reserved), FMX_EDIT_MAX_EDITS,\n"
        "         FMX_EDIT_MAX_LEN);\n"
        "  return 0;\n}\n")
    exe = tmp_path / "sizes"
    subprocess.check_call(["gcc", "-std=c99", "-Wall", "-Wextra", "-Werror", "-pedantic", "-I" + os.path.join(ROOT, "include"),
                           str(src), "-o", str(exe)])
    out = subprocess.run([str(exe)], capture_output=True, text=True, timeout=60)
    assert out.stdout.split() == ["24", "8", "4", "6", "8", "5", "6", "2", "255"]
    assert (_lib.FMX_EDIT_MAX_EDITS, _lib.FMX_EDIT_MAX_LEN) == (2, 255)


def test_abi_version_and_stats_size_stay():
    assert _lib.load().fmx_abi_version() == 5
    assert ctypes.sizeof(_lib.fmx_stats_t) == 232


def test_argument_refusals_before_any_device():
    """Everything the calls decide from their arguments alone comes before the handle is looked at, and the null handle is
    refused last with a message of its own: without a GPU, where no handle can be opened, each refusal still shows by its
    message."""
    L = _lib.load()
    n_out = ctypes.c_size_t(77)
    pat = np.frombuffer(b"abcd" * 100, dtype=np.uint8)
    off = np.array([0, 2, 4], dtype=np.uint64)
    out_off = np.zeros(3, dtype=np.uint64)
    out = np.zeros(4, dtype=[("pattern", np.uint32), ("edits", np.uint16), ("len", np.uint16), ("sp", np.uint64), ("ep", np.uint64)])

    def host(h=None, o=off, k=2, opts=None, cap=4, n=n_out, oo=out_off):
        return L.fmx_search_edit_batch(h, pat.ctypes.data, o.ctypes.data, k, ctypes.byref(opts) if opts is not None else None,
                                       oo.ctypes.data if oo is not None else None, out.ctypes.data, cap,
                                       ctypes.byref(n) if n is not None else None)

    def dev(h=None, k=2, opts=None, cap=4, n=n_out):
        return L.fmx_search_edit_batch_dev(h, pat.ctypes.data, off.ctypes.data, k, ctypes.byref(opts) if opts is not None else None,
                                           out_off.ctypes.data, out.ctypes.data, cap, ctypes.byref(n) if n is not None else None, None)

    O = _lib.fmx_edit_opts
    cases = [
        (dict(), b"handle"),
        (dict(n=None), b"n_out"),
        (dict(opts=O(3, 0, 0, 0)), b"max_edits"),
        (dict(opts=O(2 ** 32 - 1, 0, 0, 0)), b"max_edits"),
        (dict(opts=O(1, 5, 4, 0)), b"sub_lo > sub_hi"),
        (dict(opts=O(1, 0, 9, 0)), b"symbol 0"),
        (dict(opts=O(1, 9, 0, 0)), b"symbol 0"),
        (dict(opts=O(1, 1, 255, 1)), b"reserved"),
        (dict(k=(1 << 23) + 1), b"2^23"),
        (dict(cap=1 << 32), b"2^32"),
    ]
    for form in (host, dev):
        for kw, word in cases:
            assert form(**kw) == ARG, (form.__name__, kw)
            assert word in L.fmx_last_error(), (form.__name__, kw, L.fmx_last_error())
        assert form(opts=O(2, 2, 254, 0)) == ARG and b"handle" in L.fmx_last_error()         # (a valid call but for the handle)
    assert host(o=np.array([0, 3, 2], dtype=np.uint64)) == ARG and b"non-decreasing" in L.fmx_last_error()
    assert host(oo=None) == ARG and b"null argument" in L.fmx_last_error()
    # a pattern of 256 bytes: the host form sees it on the host (255 is fine: the handle is what is refused then)
    assert host(o=np.array([0, 2, 258], dtype=np.uint64)) == ARG and b"255 bytes" in L.fmx_last_error()
    assert host(o=np.array([0, 256, 258], dtype=np.uint64)) == ARG and b"255 bytes" in L.fmx_last_error()
    assert host(o=np.array([0, 2, 257], dtype=np.uint64)) == ARG and b"handle" in L.fmx_last_error()
    assert n_out.value == 77                                 # a refused call writes nothing
    a, b = ctypes.c_double(-1), ctypes.c_double(-1)
    c, d = ctypes.c_uint64(5), ctypes.c_uint64(5)
    assert L.fmx_edit_last(ctypes.byref(a), ctypes.byref(b), ctypes.byref(c), ctypes.byref(d)) == 0
    assert a.value >= 0 and b.value >= 0
    assert L.fmx_edit_last(None, None, None, None) == 0
