"""The order step's host arithmetic (findex_amd/csrc/fmx_order_math.h) under AddressSanitizer + UBSan on the CPU: the sort
workspace's bytes against the sum every call site wrote by hand, the scan scratch against the recursion that uses it, and
bits_for against the loops it replaced (tests/native/order_math.cpp)."""
import os
import shutil
import subprocess

import pytest

from conftest import ROOT


@pytest.mark.timeout(300)
def test_order_math_under_sanitizers(tmp_path):
    if not shutil.which("g++"):
        pytest.skip("no g++")
    exe = tmp_path / "order_math"
    cmd = ["g++", "-std=c++17", "-O1", "-g", "-Wall", "-Werror", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined",
           "-I" + os.path.join(ROOT, "findex_amd", "csrc"), os.path.join(ROOT, "tests", "native", "order_math.cpp"), "-o", str(exe)]
    build = subprocess.run(cmd, capture_output=True, text=True)
    if build.returncode != 0 and "sanitize" in build.stderr and "error:" not in build.stderr:
        pytest.skip("sanitizer runtime not available: " + build.stderr[-200:])
    assert build.returncode == 0, build.stderr[-2000:]
    run = subprocess.run([str(exe)], capture_output=True, text=True, timeout=200)
    assert run.returncode == 0, (run.stdout[-2000:], run.stderr[-3000:])
    assert "order math ok" in run.stdout
