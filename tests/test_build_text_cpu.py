"""Index construction from text without a device: the argument errors of fmx_bwt_from_text* / fmx_open_text (checked
before the device is touched), the no-CPU-fallback status, fmx_write_bwt against the reference's own fixture files, and
the `python -m findex_amd.index` tool's naming and refusals."""
import ctypes
import os
import subprocess
import sys

import numpy as np
import pytest

import oracle
from conftest import ROOT
from findex_amd import _lib

ERR_ARG, ERR_HIP, ERR_UNSUPPORTED = 3, 5, 6


def _gpu_count():
    n = ctypes.c_int(0)
    _lib.load().fmx_device_count(ctypes.byref(n))
    return n.value


def _call(text, length, which="host"):
    L = _lib.load()
    eof = ctypes.c_uint64()
    counts = np.zeros(256, dtype=np.int64)
    bwt = np.zeros(16, dtype=np.uint8)
    if which == "host":
        rc = L.fmx_bwt_from_text(text, length, bwt.ctypes.data, ctypes.byref(eof), counts.ctypes.data, 0)
    elif which == "open":
        h = ctypes.c_void_p()
        rc = L.fmx_open_text(text, length, 0, ctypes.byref(h))
    else:
        rc = L.fmx_bwt_from_text_dev(text, length, bwt.ctypes.data, None, ctypes.byref(eof), counts.ctypes.data, 0, None)
    return rc, L.fmx_last_error().decode()


@pytest.mark.parametrize("which", ["host", "open", "dev"])
def test_argument_errors(which):
    rc, msg = _call(None, 5, which)
    assert rc == ERR_ARG and "null" in msg
    rc, msg = _call(b"hello", 0, which)
    assert rc == ERR_ARG and "len" in msg
    rc, msg = _call(b"hello", (1 << 32) - 1, which)            # one byte over 2^32 - 2: the length alone decides
    assert rc == ERR_UNSUPPORTED and "2^32 - 2" in msg
    if which != "dev":                                          # a host text is scanned before the device is touched
        rc, msg = _call(b"he\0lo", 5, which)
        assert rc == ERR_UNSUPPORTED and "byte 0" in msg


def test_null_outputs_are_argument_errors():
    L = _lib.load()
    eof = ctypes.c_uint64()
    counts = np.zeros(256, dtype=np.int64)
    assert L.fmx_bwt_from_text(b"abc", 3, None, ctypes.byref(eof), counts.ctypes.data, 0) == ERR_ARG
    assert L.fmx_bwt_from_text(b"abc", 3, counts.ctypes.data, None, counts.ctypes.data, 0) == ERR_ARG
    assert L.fmx_open_text(b"abc", 3, 0, None) == ERR_ARG


@pytest.mark.skipif(_gpu_count() > 0, reason="checks the no-device status")
@pytest.mark.parametrize("which", ["host", "open", "dev"])
def test_valid_text_without_a_device(which):
    rc, msg = _call(b"abracadabra", 11, which)
    assert rc == ERR_HIP and "no CPU fallback" in msg


@pytest.mark.parametrize("name,be", [("words", True), ("test1024.cmp", False)])
def test_write_bwt_reproduces_the_fixture_files(testdata, tmp_path, name, be):
    import findex_amd
    bwt, size, eof = oracle.load_bwt_file(os.path.join(testdata, name + ".bwt"), bigEndian=be)
    aux = oracle.load_aux_file(os.path.join(testdata, name + ".aux"), bigEndian=be)
    b, a = tmp_path / "x.bwt", tmp_path / "x.aux"
    findex_amd.write_bwt(b, a, bwt, eof, aux, bigEndian=be)
    assert b.read_bytes() == open(os.path.join(testdata, name + ".bwt"), "rb").read()
    assert a.read_bytes() == open(os.path.join(testdata, name + ".aux"), "rb").read()
    bwt2, size2, eof2 = oracle.load_bwt_file(str(b), bigEndian=be)
    assert (size2, eof2) == (size, eof) and np.array_equal(bwt2, bwt)
    assert np.array_equal(oracle.load_aux_file(str(a), bigEndian=be), aux)


def test_written_files_open_in_the_oracle(tmp_path):
    import findex_amd
    from helpers import bwt_of_text
    text = b"mississippi banana abracadabra"
    bwt, eof, counts = bwt_of_text(text[::-1])
    for be in (True, False):
        b, a = tmp_path / ("t%d.bwt" % be), tmp_path / ("t%d.aux" % be)
        findex_amd.write_bwt(b, a, bwt, eof, counts, bigEndian=be)
        s = oracle.NaiveFMSearcher(str(b), bigEndian=be)
        assert s.n == len(text) + 1 and s.eof == eof
        r = s.search(b"ssi"[::-1])
        assert r is not None and r[1] - r[0] == 2


def test_write_bwt_argument_errors(tmp_path):
    L = _lib.load()
    bwt = np.zeros(4, dtype=np.uint8)
    counts = np.zeros(256, dtype=np.int64)
    p = str(tmp_path / "x.bwt").encode()
    assert L.fmx_write_bwt(None, p, bwt.ctypes.data, 4, 0, counts.ctypes.data, 1) == ERR_ARG
    assert L.fmx_write_bwt(p, p, bwt.ctypes.data, 4, 4, counts.ctypes.data, 1) == ERR_ARG          # eof >= n
    assert L.fmx_write_bwt(b"/nonexistent/x.bwt", p, bwt.ctypes.data, 4, 0, counts.ctypes.data, 1) == 1


def test_cli_names_outputs_like_the_reference():
    from findex_amd.index import output_names
    assert output_names("/a/b/words.txt") == ("/a/b/words.bwt", "/a/b/words.aux")
    assert output_names("x.y.txt") == ("x.y.bwt", "x.y.aux")
    assert output_names("plain") == ("plain.bwt", "plain.aux")


def _cli(*args):
    env = dict(os.environ)
    env["PYTHONPATH"] = ROOT + os.pathsep + env.get("PYTHONPATH", "")
    return subprocess.run([sys.executable, "-m", "findex_amd.index"] + list(args), cwd=ROOT, env=env,
                          capture_output=True, text=True, timeout=300)


def test_cli_refuses_byte_0(tmp_path):
    p = tmp_path / "z.txt"
    p.write_bytes(b"abc\0def")
    r = _cli(str(p))
    assert r.returncode != 0 and "byte 0" in r.stderr and "offset 3" in r.stderr
    assert not (tmp_path / "z.bwt").exists() and not (tmp_path / "z.aux").exists()


@pytest.mark.skipif(_gpu_count() > 0, reason="checks the no-device status")
def test_cli_without_a_device_fails_loudly(tmp_path):
    p = tmp_path / "t.txt"
    p.write_bytes(b"abracadabra")
    r = _cli(str(p))
    assert r.returncode != 0 and "no CPU fallback" in r.stderr
    assert not (tmp_path / "t.bwt").exists()
