"""Matching statistics and MEMs without a device: the two expectations of tests/mstat_ref.py against each other, the
layout of the two new structs against a strict-C compile of the header, the new symbols, and every refusal the calls decide
on the host."""
import ctypes
import itertools
import os
import re
import shutil
import subprocess

import numpy as np
import pytest

import approx_ref
import mstat_ref
from conftest import ROOT
from findex_amd import _lib
from helpers import pack_patterns

ARG = 3
NEW = ("fmx_match_stats_batch", "fmx_match_stats_batch_dev", "fmx_mems_batch", "fmx_mems_batch_dev", "fmx_mstat_last")


def tiny():
    rng = np.random.default_rng(7)
    s = bytes(rng.integers(97, 100, 60, dtype=np.uint8))          # sigma = 3
    pats = [bytes(P) for m in range(1, 6) for P in itertools.product(b"abc", repeat=m)]
    return s, approx_ref.index_of(s)[0], pats


def test_the_two_references_agree_on_tiny_texts():
    """Every pattern over abc up to 5 bytes, in batches of several patterns with empty ones between, caps 1, 2, 3 (and 64,
    which never binds): the loop over getPrevRange, in its batched and its scalar form, equals the substring test; the MEM
    rule gives each pattern's last byte whenever its length reaches min_len."""
    s, orc, pats = tiny()
    assert len(pats) == 363
    hits = 0
    for at in range(0, len(pats), 40):
        batch = []
        for p in pats[at:at + 40]:
            batch += [p, b""] if len(batch) % 3 == 0 else [p]
        buf, off = pack_patterns(batch)
        for cap in (1, 2, 3, 64):
            ln, sp, ep, steps = mstat_ref.loop_stats(orc, buf, off, cap)
            assert np.array_equal(ln, mstat_ref.brute_stats(s, buf, off, cap)), (at, cap)
            for got, want in zip(mstat_ref.text_stats(orc, s, buf, off, cap), (ln, sp, ep, steps)):
                assert np.array_equal(got, want), (at, cap)
            l2, s2, e2, st2 = mstat_ref.loop_stats_scalar(orc, buf, off, cap)
            assert ln.tolist() == l2 and sp.tolist() == s2 and ep.tolist() == e2 and steps.tolist() == st2, (at, cap)
            _, e, L = mstat_ref.limits(off, buf.size, cap)
            assert (ln <= L).all() and ((steps == ln) | (steps == ln + 1)).all() and (steps[ln == L] == L[ln == L]).all()
            for j in np.nonzero(ln)[0].tolist():             # the interval is the exact search's for that suffix
                assert orc.search(bytes(buf[j - int(ln[j]) + 1:j + 1])) == (int(sp[j]), int(ep[j]))
            assert all((int(sp[j]), int(ep[j])) == (0, orc.n) for j in np.nonzero(ln == 0)[0].tolist())
            out_off, rows = mstat_ref.mems_of(ln, off, 1)
            assert out_off[-1] == len(rows) and len(out_off) == off.size
            ends = {(q, end) for q, _, end in rows}
            for q in range(off.size - 1):
                if off[q + 1] > off[q] and ln[int(off[q + 1]) - 1] >= 1:
                    assert (q, int(off[q + 1] - off[q])) in ends
            hits += len(rows)
    assert hits > 1000


def test_a_length_grows_by_one_at_most():
    s, orc, pats = tiny()
    rng = np.random.default_rng(3)
    q = bytearray(s[5:45])
    q[20] = 100                                              # 'd': not in the text
    batch = [bytes(q), s[10:30] + s[2:17], bytes(rng.integers(97, 100, 80, dtype=np.uint8))]
    buf, off = pack_patterns(batch)
    for cap in (1, 3, 7, 64):
        ln = mstat_ref.loop_stats(orc, buf, off, cap)[0].astype(np.int64)
        assert (ln[1:] <= ln[:-1] + 1).all()
        assert np.array_equal(ln, mstat_ref.brute_stats(s, buf, off, cap))
        assert ln[20] == 0 and ln[19] == min(20, cap)
    # byte 0 in a pattern: the loop treats it as the exact search does
    buf, off = pack_patterns([s[-4:] + b"\0", b"\0" + s[:3], b"a\0b"])
    ln, sp, ep, _ = mstat_ref.loop_stats(orc, buf, off, 64)
    for j in range(buf.size):
        q = int(np.searchsorted(off, j, side="right") - 1)
        for l in range(1, j - int(off[q]) + 2):
            r = orc.search(bytes(buf[j - l + 1:j + 1]))
            assert (r is not None) == (l <= ln[j]), (j, l)
            if l == ln[j]:
                assert r == (int(sp[j]), int(ep[j]))


def test_struct_layouts():
    assert ctypes.sizeof(_lib.fmx_mem_hit) == 32 and ctypes.sizeof(_lib.fmx_mstat_opts) == 16
    H = _lib.fmx_mem_hit
    assert (H.pattern.offset, H.len.offset, H.end.offset, H.sp.offset, H.ep.offset) == (0, 4, 8, 16, 24)
    O = _lib.fmx_mstat_opts
    assert (O.max_len.offset, O.min_len.offset, O.reserved.offset) == (0, 4, 8)
    import findex_amd
    M = findex_amd.HipFMSearcher.MEM_HIT
    assert M.itemsize == 32 and [M.fields[f][1] for f in ("pattern", "len", "end", "sp", "ep")] == [0, 4, 8, 16, 24]


@pytest.mark.skipif(shutil.which("gcc") is None, reason="needs gcc")
def test_struct_layouts_against_a_strict_c_compile(tmp_path):
    src = tmp_path / "sizes.c"
    src.write_text(
        "#include <stddef.h>\n#include <stdio.h>\n#include <fmx.h>\n"
        "int main(void) {\n"
        "  printf(\"%d %d %d %d %d %d %d %d %d %d\\n\", (int)sizeof(fmx_mem_hit), (int)sizeof(fmx_mstat_opts),\n"
        "         (int)offsetof(fmx_mem_hit, len), (int)offsetof(fmx_mem_hit, end), (int)offsetof(fmx_mem_hit, sp),\n"
        "         (int)offsetof(fmx_mem_hit, ep), (int)offsetof(fmx_mstat_opts, min_len),\n"
        "         (int)offsetof(fmx_mstat_opts, reserved), FMX_MSTAT_MAX_LEN, FMX_MSTAT_TILE);\n"
        "  return 0;\n}\n")
    exe = tmp_path / "sizes"
    subprocess.check_call(["gcc", "-std=c99", "-Wall", "-Wextra", "-Werror", "-pedantic", "-I" + os.path.join(ROOT, "include"),
                           str(src), "-o", str(exe)])
    out = subprocess.run([str(exe)], capture_output=True, text=True, timeout=60)
    assert out.stdout.split() == ["32", "16", "4", "8", "16", "24", "4", "8", str(_lib.FMX_MSTAT_MAX_LEN), str(_lib.FMX_MSTAT_TILE)]
    assert _lib.FMX_MSTAT_MAX_LEN == 4096


def test_symbols_are_declared_bound_and_exported():
    with open(os.path.join(ROOT, "include", "fmx.h")) as f:
        header = f.read()
    L = _lib.load()
    for name in NEW:
        assert re.search(r"\bint %s\(" % name, header), name
        assert name in _lib.SYMBOLS and getattr(L, name).argtypes == _lib.SYMBOLS[name][1], name
    assert len(_lib.SYMBOLS["fmx_match_stats_batch_dev"][1]) == 10 and len(_lib.SYMBOLS["fmx_mems_batch_dev"][1]) == 11
    assert L.fmx_abi_version() == 5
    assert ctypes.sizeof(_lib.fmx_stats_t) == 232


def test_argument_refusals_before_any_device():
    """Everything the calls decide from their arguments alone comes before the handle is looked at, and the null handle is
    refused last with a message of its own: on a machine without a GPU, where no handle can be opened, each refusal still
    shows by its message."""
    L = _lib.load()
    n_out = ctypes.c_size_t(77)
    pat = np.frombuffer(b"abcd", dtype=np.uint8)
    off = np.array([0, 2, 4], dtype=np.uint64)
    ln = np.full(4, 9, dtype=np.uint32)
    sp = np.zeros(4, dtype=np.uint64)
    out_off = np.full(3, 9, dtype=np.uint64)
    out = np.zeros(4, dtype=[("pattern", np.uint32), ("len", np.uint32), ("end", np.uint64), ("sp", np.uint64), ("ep", np.uint64)])
    by = ctypes.byref

    def p(a):
        return a.ctypes.data if a is not None else None

    def stats(h=None, o=off, k=2, opts=None, l=ln):
        return L.fmx_match_stats_batch(h, p(pat), p(o), k, by(opts) if opts is not None else None, p(l), p(sp), None)

    def stats_dev(h=None, k=2, nb=4, opts=None, l=ln):
        return L.fmx_match_stats_batch_dev(h, p(pat), p(off), k, nb, by(opts) if opts is not None else None, p(l), None, None, None)

    def mems(h=None, o=off, k=2, opts=None, cap=4, n=n_out, oo=out_off):
        return L.fmx_mems_batch(h, p(pat), p(o), k, by(opts) if opts is not None else None, p(oo), p(out), cap,
                                by(n) if n is not None else None)

    def mems_dev(h=None, k=2, nb=4, opts=None, cap=4, n=n_out, oo=out_off):
        return L.fmx_mems_batch_dev(h, p(pat), p(off), k, nb, by(opts) if opts is not None else None, p(oo), p(out), cap,
                                    by(n) if n is not None else None, None)

    O = _lib.fmx_mstat_opts
    common = [
        (dict(), b"handle"),
        (dict(opts=O(4097, 0, (0, 0))), b"max_len"),
        (dict(opts=O(2 ** 32 - 1, 0, (0, 0))), b"max_len"),
        (dict(opts=O(7, 8, (0, 0))), b"min_len > max_len"),
        (dict(opts=O(0, 4097, (0, 0))), b"min_len > max_len"),
        (dict(opts=O(7, 1, (1, 0))), b"reserved"),
        (dict(opts=O(7, 1, (0, 1))), b"reserved"),
        (dict(k=(1 << 26) + 1), b"2^26"),
    ]
    for form in (stats, stats_dev, mems, mems_dev):
        for kw, word in common:
            assert form(**kw) == ARG, (form.__name__, kw)
            assert word in L.fmx_last_error(), (form.__name__, kw, L.fmx_last_error())
    for form in (stats, stats_dev):
        assert form(l=None) == ARG and b"null" in L.fmx_last_error()
    for form in (mems, mems_dev):
        assert form(cap=1 << 32) == ARG and b"cap" in L.fmx_last_error()
        assert form(n=None) == ARG and b"n_out" in L.fmx_last_error()
        assert form(oo=None) == ARG and b"null argument" in L.fmx_last_error()
    for form in (stats_dev, mems_dev):
        assert form(nb=1 << 32) == ARG and b"n_bytes" in L.fmx_last_error()
    big = np.array([0, 2, 1 << 32], dtype=np.uint64)
    for form in (stats, mems):
        assert form(o=np.array([0, 3, 2], dtype=np.uint64)) == ARG and b"non-decreasing" in L.fmx_last_error()
        assert form(o=np.array([1, 2, 4], dtype=np.uint64)) == ARG and b"off[0]" in L.fmx_last_error()
        assert form(o=big) == ARG and b"n_bytes" in L.fmx_last_error()
    # a refused call writes nothing
    assert n_out.value == 77 and (ln == 9).all() and (out_off == 9).all()
    a, b = ctypes.c_double(-1), ctypes.c_double(-1)
    c, d = ctypes.c_uint64(5), ctypes.c_uint64(5)
    assert L.fmx_mstat_last(by(a), by(b), by(c), by(d)) == 0
    assert a.value >= 0 and b.value >= 0 and c.value == 0 and d.value == 0
    assert L.fmx_mstat_last(None, None, None, None) == 0
