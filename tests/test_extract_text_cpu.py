"""Extraction by text position without a device: the new symbols, the "extract_sample" key, every refusal the calls decide
on the host, and the piece walk of tests/extract_ref.py over the oracle's LF against slicing the text, with its step bounds."""
import ctypes
import os
import re

import numpy as np

import approx_ref
import extract_ref
from conftest import ROOT
from findex_amd import _lib
from helpers import bwt_of_text

ARG = 3
NEW = ("fmx_extract_text_batch", "fmx_extract_text_batch_dev", "fmx_extract_info", "fmx_extract_last")


def test_symbols_are_declared_bound_and_exported():
    with open(os.path.join(ROOT, "include", "fmx.h")) as f:
        header = f.read()
    code = re.sub(r"/\*.*?\*/", "", header, flags=re.S)
    L = _lib.load()
    for name in NEW:
        assert re.search(r"\bint %s\(" % name, code), name
        assert name in _lib.SYMBOLS and getattr(L, name).argtypes == _lib.SYMBOLS[name][1], name
    assert len(_lib.SYMBOLS["fmx_extract_text_batch"][1]) == 5 and len(_lib.SYMBOLS["fmx_extract_text_batch_dev"][1]) == 7
    assert re.search(r"FMX_PREPARE_EXTRACT\s*=\s*128\b", code)
    tile = re.search(r"#define\s+FMX_EXTRACT_TILE\s+(\d+)", code)
    assert tile and int(tile.group(1)) == _lib.FMX_EXTRACT_TILE
    assert L.fmx_abi_version() == 5
    assert ctypes.sizeof(_lib.fmx_stats_t) == 232


def test_extract_sample_takes_its_values_and_refuses_others():
    L = _lib.load()
    try:
        for v in (b"1", b"32", b"4096"):
            assert L.fmx_config_set(b"extract_sample", v) == 0, v
        for v in (b"0", b"4097", b"text", b"", b"-1", b"32x", b"3.5"):
            assert L.fmx_config_set(b"extract_sample", v) == ARG, v
            assert b"extract_sample" in L.fmx_last_error()
        # the per-handle call refuses a null handle before it looks at the value; a handle's own values need a device
        for v in (b"0", b"4097", b"text", b"32"):
            assert L.fmx_index_config_set(None, b"extract_sample", v) == ARG, v
    finally:
        assert L.fmx_config_set(b"extract_sample", b"32") == 0
    # locate's key is its own
    assert L.fmx_config_set(b"locate_sample", b"32") == 0


def test_argument_refusals_before_any_device():
    """Everything the calls decide from their arguments alone comes before the handle is looked at, and the null handle is
    refused last with a message of its own: on a machine without a GPU, where no handle can be opened, each refusal still
    shows by its message.  (pos + length > n - 1 needs a handle: tests/test_gpu_extract.py.)"""
    L = _lib.load()
    pos = np.array([0, 5], dtype=np.uint64)
    off = np.array([0, 2, 4], dtype=np.uint64)
    out = np.full(4, 9, dtype=np.uint8)

    def p(a):
        return a.ctypes.data if a is not None else None

    def host(h=None, ps=pos, o=off, k=2, dst=out):
        return L.fmx_extract_text_batch(h, p(ps), p(o), k, p(dst))

    def dev(h=None, ps=pos, o=off, k=2, nb=4, dst=out):
        return L.fmx_extract_text_batch_dev(h, p(ps), p(o), k, nb, p(dst), None)

    for form in (host, dev):
        assert form() == ARG and b"handle" in L.fmx_last_error(), form.__name__
        assert form(k=(1 << 26) + 1) == ARG and b"2^26" in L.fmx_last_error(), form.__name__
        assert form(ps=None) == ARG and b"null" in L.fmx_last_error(), form.__name__
        assert form(o=None) == ARG and b"null" in L.fmx_last_error(), form.__name__
        assert form(dst=None) == ARG and b"null" in L.fmx_last_error(), form.__name__
    assert host(o=np.array([1, 2, 4], dtype=np.uint64)) == ARG and b"off[0]" in L.fmx_last_error()
    assert host(o=np.array([0, 3, 2], dtype=np.uint64)) == ARG and b"non-decreasing" in L.fmx_last_error()
    assert host(o=np.array([0, 2, 1 << 32], dtype=np.uint64)) == ARG and b"n_bytes" in L.fmx_last_error()
    assert dev(nb=1 << 32) == ARG and b"n_bytes" in L.fmx_last_error()
    # k == 0 and empty batches still want a handle
    assert host(k=0) == ARG and b"handle" in L.fmx_last_error()
    assert dev(k=0, nb=0) == ARG and b"handle" in L.fmx_last_error()
    assert (out == 9).all()                                   # a refused call writes nothing
    rate, nbytes, ms = ctypes.c_uint32(), ctypes.c_uint64(), ctypes.c_double()
    assert L.fmx_extract_info(None, ctypes.byref(rate), ctypes.byref(nbytes), ctypes.byref(ms)) == ARG
    assert L.fmx_prepare(None, 128) == ARG and L.fmx_drop_tables(None, 128) == ARG
    a, b, c = ctypes.c_double(-1), ctypes.c_uint64(5), ctypes.c_uint64(5)
    assert L.fmx_extract_last(ctypes.byref(a), ctypes.byref(b), ctypes.byref(c)) == 0
    assert a.value >= 0 and b.value == 0 and c.value == 0
    assert L.fmx_extract_last(None, None, None) == 0


def _index(text):
    """(BWT', LF) of the index of `text` as from_text has it: the BWT of reverse(text) + sentinel, by the oracle."""
    s = bytes(text[::-1])
    orc = approx_ref.index_of(s)[0]
    bwt, eof, _ = bwt_of_text(s)
    assert orc.eof == eof and orc.n == len(text) + 1
    return extract_ref.index_arrays(orc, bwt)


RATES = (1, 2, 3, 7, 32)


def test_piece_walk_against_slicing():
    """Every (offset, length) of random texts over small alphabets at rates 1, 2, 3, 7, 32 (and one above n): byte-equal to
    the slice, no walk longer than 2 s - 1, and the samples the same by the inversion and by the scatter."""
    rng = np.random.default_rng(17)
    texts = [bytes(rng.integers(97, 97 + int(rng.integers(1, 5)), int(rng.integers(1, 41)), dtype=np.uint8)) for _ in range(12)]
    texts += [b"a", b"ab", b"aaaaaaaaaaaaaaaaaaaaaaaaaaaaaaaaa", b"abracadabra" * 3]
    ranges = 0
    for text in texts:
        bwt, lf = _index(text)
        n = len(text) + 1
        for s in RATES + (n + 5,):
            isa = extract_ref.isa_samples(lf, s)
            assert isa == extract_ref.isa_from_locate_samples(lf, s), (text, s)
            assert len(isa) == (n - 1) // s + 1 and isa[0] == bwt.index(0)          # SA 0 is the EOF row
            for a in range(len(text) + 1):
                for ln in range(len(text) - a + 1):
                    got, steps, _, longest = extract_ref.extract_batch(bwt, lf, isa, s, [a], [ln])
                    assert got == text[a:a + ln], (text, s, a, ln)
                    assert longest <= 2 * s - 1 and ln <= steps
                    ranges += 1
    assert ranges > 20000


def test_batches_tiles_and_step_bounds():
    """Batches with empty ranges and tile cuts of the output: the bytes are the slices back to back, and the steps keep
    the bounds of fmx.h whatever the tile."""
    rng = np.random.default_rng(18)
    text = bytes(rng.integers(97, 100, 70, dtype=np.uint8))
    bwt, lf = _index(text)
    pairs = [(a, ln) for a in range(71) for ln in range(71 - a)]
    assert len(pairs) == 2556
    pos = [a for a, _ in pairs]
    lens = [ln for _, ln in pairs]
    want = b"".join(text[a:a + ln] for a, ln in pairs)
    for s in (1, 3, 32, 4096):
        isa = extract_ref.isa_samples(lf, s)
        for tile in (1, 7, 64, 1024, 1 << 60):
            got, steps, n_pieces, longest = extract_ref.extract_batch(bwt, lf, isa, s, pos, lens, tile)
            assert got == want, (s, tile)
            lo, hi = extract_ref.step_bounds(s, lens, tile)
            assert lo == len(want) and lo <= steps <= hi, (s, tile, lo, steps, hi)
            assert longest <= 2 * s - 1
            if s == 1:
                assert steps == lo                           # every byte is a sample: nothing is ever skipped
