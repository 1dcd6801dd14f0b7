"""Occurrences without a device (fmx_occurrences): the expectations of tests/occ_ref.py against each other on
the word text, hand-worked cases, the layout of the two structs against a strict-C compile of the header, and every refusal
the calls decide on the host.  What needs a handle is in tests/test_gpu_occurrences.py: no handle opens without a device."""
import ctypes
import os
import shutil
import subprocess

import numpy as np
import pytest

import corpus_ref
import occ_ref
from conftest import ROOT
from findex_amd import _lib

ARG = 3


def interval(orc, Q):
    """The rows of the text string Q: the index holds the reversed text."""
    r = orc.search(bytes(Q)[::-1])
    assert r is not None, Q
    return int(r[0]), int(r[1])


def pairs(csr, g=None):
    off, occ = csr
    sel = occ if g is None else occ[int(off[g]):int(off[g + 1])]
    return [(int(o["pos"]), int(o["len"])) for o in sel]


def test_the_references_agree_on_the_word_text():
    """brute_regex (no index) equals the oracle's frontier through from_records, in the three modes; the counts are not
    trivial, and for b.*b the longest reading really has fewer elements than the full one."""
    T = occ_ref.word_text()
    orc, sa = occ_ref.oracle_index(T)
    tabs = occ_ref.regex_tables()
    counts = {}
    for mode in ("all", "longest", "disjoint"):
        b = occ_ref.brute_csr(tabs, T, occ_ref.MAX_LEN, mode)
        f = occ_ref.from_frontier(orc, tabs, sa, T, occ_ref.MAX_LEN, mode)
        assert np.array_equal(b[0], f[0]), mode
        assert b[1].tobytes() == f[1].tobytes(), mode
        counts[mode] = np.diff(b[0]).astype(np.int64).tolist()
    print("ALL pairs per regex: %s" % dict(zip(occ_ref.REGEXES, counts["all"])))
    assert all(c > 100 for m in counts.values() for c in m)
    i = occ_ref.REGEXES.index("b.*b")
    assert counts["disjoint"][i] < counts["longest"][i] < counts["all"][i]
    assert counts["longest"][occ_ref.REGEXES.index("ab")] == counts["all"][occ_ref.REGEXES.index("ab")]
    # the isLast rule: ab* stops at the a
    assert set(ln for _, ln in pairs(b, occ_ref.REGEXES.index("ab*"))) == {1}


def test_hand_worked_cases():
    T = b"aaaaa"
    orc, sa = occ_ref.oracle_index(T)
    aa, aaa = interval(orc, b"aa"), interval(orc, b"aaa")
    assert aa[1] - aa[0] == 4 and aaa[1] - aaa[0] == 3
    one = [(0, 2) + aa, (0, 3) + aaa]
    assert pairs(occ_ref.from_records(T, sa, one, "all")) == [(0, 2), (0, 3), (1, 2), (1, 3), (2, 2), (2, 3), (3, 2)]
    assert pairs(occ_ref.from_records(T, sa, one, "longest")) == [(0, 3), (1, 3), (2, 3), (3, 2)]
    assert pairs(occ_ref.from_records(T, sa, one, "disjoint")) == [(0, 3), (3, 2)]
    two = [(0, 2) + aa, (1, 3) + aaa]
    d = occ_ref.from_records(T, sa, two, "disjoint")
    assert d[0].tolist() == [0, 2, 3] and pairs(d, 0) == [(0, 2), (2, 2)] and pairs(d, 1) == [(0, 3)]
    assert occ_ref.from_records(T, sa, two, "all")[0].tolist() == [0, 4, 7]
    # a duplicate record is merged, an empty one and one of length 0 have no occurrences, a group without records is empty
    dup = [(2, 2) + aa, (2, 2) + aa, (0, 2, 3, 3), (0, 0) + aa]
    a = occ_ref.from_records(T, sa, dup, "all")
    assert a[0].tolist() == [0, 0, 0, 4] and pairs(a, 2) == [(0, 2), (1, 2), (2, 2), (3, 2)]
    # max_per = 1: the first row of each record alone
    m1 = occ_ref.from_records(T, sa, one, "all", max_per=1)
    assert pairs(m1) == sorted([(5 - 2 - int(sa[aa[0]]), 2), (5 - 3 - int(sa[aaa[0]]), 3)])
    assert m1[1]["doc"].tolist() == [0xFFFFFFFF] * 2 and m1[1]["raw_off"].tolist() == m1[1]["pos"].tolist()


def test_hand_worked_corpus_case():
    """Three documents, one empty, one with raw 0 / 1 / 255: a record whose string holds the separator is dropped before the
    reduction, so the shorter one at its start wins under LONGEST; raw offsets and lengths count raw bytes."""
    docs = corpus_ref.RefCorpus([b"ab\x00c", b"", b"ab\x01\xffab"])
    S = docs.stream
    assert S == b"ab\\0c\x01\x01ab\\1\\fab\x01" and docs.doc_start == [0, 6, 7, 16]
    orc, sa = occ_ref.oracle_index(S)
    c1, c = interval(orc, b"c\x01"), interval(orc, b"c")
    recs = [(0, 2) + c1, (0, 1) + c, (1, 2) + interval(orc, b"ab"), (1, 3) + interval(orc, b"b\\0"),
            (1, 5) + interval(orc, b"b\\1\\f"), (1, 3) + interval(orc, b"\x01ab")]
    without = occ_ref.from_records(S, sa, recs, "longest")
    assert pairs(without, 0) == [(4, 2)]
    with_ = occ_ref.from_records(S, sa, recs, "longest", docs=docs)
    assert pairs(with_, 0) == [(4, 1)]
    o = with_[1][0]
    assert (int(o["doc"]), int(o["raw_off"]), int(o["raw_len"])) == (0, 3, 1)
    g1 = with_[1][int(with_[0][1]):]
    # ab at stream 0, 7, 13; b\0 at 1 (the end falls on the escape's second byte: raw bytes 1 .. 2); b\1\f at 8 (raw 1 .. 3);
    # \x01ab spans the separator in front of document 2 and is dropped
    assert [(int(x["pos"]), int(x["len"]), int(x["doc"]), int(x["raw_off"]), int(x["raw_len"])) for x in g1] == \
        [(0, 2, 0, 0, 2), (1, 3, 0, 1, 2), (7, 2, 2, 0, 2), (8, 5, 2, 1, 3), (13, 2, 2, 4, 2)]
    assert 6 in [p for p, _ in pairs(without, 1)] and 6 not in [p for p, _ in pairs(with_, 1)]


def test_struct_layouts():
    assert ctypes.sizeof(_lib.fmx_occurrence) == 32 and ctypes.sizeof(_lib.fmx_occ_opts) == 16
    O = _lib.fmx_occurrence
    assert [getattr(O, f).offset for f in ("group", "len", "pos", "doc", "raw_len", "raw_off")] == [0, 4, 8, 16, 20, 24]
    assert _lib.fmx_occ_opts.reserved.offset == 4 and _lib.fmx_occ_opts.max_per.offset == 8
    import findex_amd
    H = findex_amd.HipFMSearcher
    assert H.OCCURRENCE.itemsize == 32 and H.RESULT.itemsize == 24 and H.OCCURRENCE == occ_ref.OCC
    assert [H.OCCURRENCE.fields[f][1] for f in ("group", "len", "pos", "doc", "raw_len", "raw_off")] == [0, 4, 8, 16, 20, 24]


@pytest.mark.skipif(shutil.which("gcc") is None, reason="needs gcc")
def test_struct_layouts_against_a_strict_c_compile(tmp_path):
    src = tmp_path / "sizes.c"
    src.write_text(
        "#include <stddef.h>\n#include <stdio.h>\n#include <fmx.h>\n"
        "int main(void) {\n"
        "  printf(\"%d %d %d %d %d %d %d %d %d %u %u %u %d\\n\", (int)sizeof(fmx_occurrence), (int)sizeof(fmx_occ_opts),\n"
        "         (int)offsetof(fmx_occurrence, len), (int)offsetof(fmx_occurrence, pos), (int)offsetof(fmx_occurrence, doc),\n"
        "         (int)offsetof(fmx_occurrence, raw_len), (int)offsetof(fmx_occurrence, raw_off),\n"
        "         (int)offsetof(fmx_occ_opts, reserved), (int)offsetof(fmx_occ_opts, max_per), FMX_OCC_ALL, FMX_OCC_LONGEST,\n"
        "         FMX_OCC_DISJOINT, FMX_OCC_MAX_LEN);\n"
        "  return 0;\n}\n")
    exe = tmp_path / "sizes"
    subprocess.check_call(["gcc", "-std=c99", "-Wall", "-Wextra", "-Werror", "-pedantic", "-I" + os.path.join(ROOT, "include"),
                           str(src), "-o", str(exe)])
    out = subprocess.run([str(exe)], capture_output=True, text=True, timeout=60)
    assert out.stdout.split() == ["32", "16", "4", "8", "16", "20", "24", "4", "8", "0", "1", "2", "65535"]
    assert (_lib.FMX_OCC_ALL, _lib.FMX_OCC_LONGEST, _lib.FMX_OCC_DISJOINT, _lib.FMX_OCC_MAX_LEN) == (0, 1, 2, 65535)


def test_abi_version_and_stats_size_stay():
    assert _lib.load().fmx_abi_version() == 5
    assert ctypes.sizeof(_lib.fmx_stats_t) == 232


def test_argument_refusals_before_any_device():
    """Everything the calls decide from their arguments alone comes before the handle is looked at, and the null handle is
    refused last with a message of its own: without a GPU, where no handle can be opened, each refusal still shows by its
    message."""
    import findex_amd
    L = _lib.load()
    n_out = ctypes.c_size_t(77)
    rec = findex_amd.HipFMSearcher.pack_records([0, 1], [2, 3], [5, 6], [7, 9])
    out_off = np.full(3, 99, dtype=np.uint64)
    out = np.zeros(4, dtype=occ_ref.OCC)

    def host(h=None, r=rec, k=2, g=2, opts=None, cap=4, n=n_out, oo=out_off, o=out):
        return L.fmx_occurrences(h, None, r.ctypes.data if r is not None else None, k, g,
                                 ctypes.byref(opts) if opts is not None else None, oo.ctypes.data if oo is not None else None,
                                 o.ctypes.data if o is not None else None, cap, ctypes.byref(n) if n is not None else None)

    def dev(h=None, r=rec, k=2, g=2, opts=None, cap=4, n=n_out, oo=out_off, o=out):
        return L.fmx_occurrences_dev(h, None, r.ctypes.data if r is not None else None, k, g,
                                     ctypes.byref(opts) if opts is not None else None, oo.ctypes.data if oo is not None else None,
                                     o.ctypes.data if o is not None else None, cap, ctypes.byref(n) if n is not None else None, None)

    O = _lib.fmx_occ_opts
    cases = [
        (dict(), b"handle"),
        (dict(n=None), b"n_out"),
        (dict(oo=None), b"out_off"),
        (dict(opts=O(3, 0, 0)), b"mode"),
        (dict(opts=O(2 ** 32 - 1, 0, 0)), b"mode"),
        (dict(opts=O(2, 1, 0)), b"reserved"),
        (dict(k=(1 << 26) + 1), b"2^26 records"),
        (dict(g=0), b"n_groups"),
        (dict(g=(1 << 26) + 1), b"n_groups"),
        (dict(cap=1 << 32), b"2^32"),
        (dict(r=None), b"records are null"),
        (dict(o=None), b"out is null"),
    ]
    for form in (host, dev):
        for kw, word in cases:
            assert form(**kw) == ARG, (form.__name__, kw)
            assert word in L.fmx_last_error(), (form.__name__, kw, L.fmx_last_error())
        assert form(opts=O(2, 0, 5)) == ARG and b"handle" in L.fmx_last_error()              # (a valid call but for the handle)
        assert form(o=None, cap=0) == ARG and b"handle" in L.fmx_last_error()                 # the counting call's shape is fine
    # the records: the host form sees them on the host
    P = findex_amd.HipFMSearcher.pack_records
    assert host(r=P([0, 2], [2, 3], [5, 6], [7, 9])) == ARG and b"group" in L.fmx_last_error()
    assert host(r=P([0, 1], [2, 65536], [5, 6], [7, 9])) == ARG and b"65535" in L.fmx_last_error()
    assert host(r=P([0, 1], [2, 3], [8, 6], [7, 9])) == ARG and b"sp > ep" in L.fmx_last_error()
    assert host(r=P([0, 1], [2, 65535], [7, 9], [7, 9])) == ARG and b"handle" in L.fmx_last_error()
    assert n_out.value == 77 and out_off.tolist() == [99, 99, 99]      # a refused call writes nothing
    t = [ctypes.c_double(-1) for _ in range(4)]
    rows = ctypes.c_uint64(5)
    assert L.fmx_occurrences_last(*[ctypes.byref(x) for x in t], ctypes.byref(rows)) == 0
    assert all(x.value >= 0 for x in t)
    assert L.fmx_occurrences_last(None, None, None, None, None) == 0
    # the mirror refuses what it can name
    with pytest.raises(ValueError):
        findex_amd.HipFMSearcher._occ_opts("shortest", None)
    with pytest.raises(ValueError):
        findex_amd.HipFMSearcher._occ_opts("all", 0)
