"""Index construction from raw text (libfmx: fmx_bwt_from_text*, fmx_write_bwt) -- the drop-in for findex's
BWTMerger2.merge over a FileBWTReader (bwtmerger.scala:654-1261), which writes X.bwt / X.aux of the REVERSED file
(copyReverse, :1106-1108).  The suffix sort runs on the device; there is no CPU fallback."""
import ctypes

import numpy as np

from . import _lib


def _text_array(text):
    if isinstance(text, (bytes, bytearray, memoryview)):
        return np.frombuffer(bytes(text), dtype=np.uint8)
    return np.ascontiguousarray(text, dtype=np.uint8).reshape(-1)


def _ptr(a):
    return a.ctypes.data_as(ctypes.c_void_p) if a is not None and a.size else None


def bwt_from_text(text, device=0):
    """fmx_bwt_from_text: the BWT of reverse(text) + EOF as findex's merger writes it.  `text` is bytes or a uint8
    array without byte 0.  Returns (bwt uint8[len + 1], eof, counts int64[256])."""
    L = _lib.load()
    t = _text_array(text)
    bwt = np.empty(t.size + 1, dtype=np.uint8)
    counts = np.zeros(256, dtype=np.int64)
    eof = ctypes.c_uint64()
    _lib.check(L.fmx_bwt_from_text(_ptr(t), t.size, _ptr(bwt), ctypes.byref(eof), _ptr(counts), int(device)))
    return bwt, int(eof.value), counts


def bwt_from_text_chunked(text, chunk, device=0):
    """The same (bwt, eof, counts) as bwt_from_text, built `chunk` bytes at a time: the first chunk by the suffix sort, every
    further one appended to the index on the device (fmx_append_text) -- the way to a text beyond 2^32 - 2 bytes."""
    from .searcher import HipFMSearcher
    hip = HipFMSearcher.from_text(_text_array(text), device=device, chunk=int(chunk))
    try:
        return hip.bwt_bytes(), hip.eof, hip.counts()
    finally:
        hip.close()


def bwt_from_text_dev(d_text, length, d_bwt, d_sa=0, device=0, stream=0):
    """fmx_bwt_from_text_dev: device pointers (e.g. tensor.data_ptr()) -- text[length] in, bwt[length + 1] out, and
    the suffix array of reverse(text) + sentinel (u32[length + 1]) into d_sa when it is not 0.  Synchronises `stream`.
    Returns (eof, counts int64[256])."""
    L = _lib.load()
    counts = np.zeros(256, dtype=np.int64)
    eof = ctypes.c_uint64()
    _lib.check(L.fmx_bwt_from_text_dev(ctypes.c_void_p(int(d_text) or None), int(length),
                                       ctypes.c_void_p(int(d_bwt) or None), ctypes.c_void_p(int(d_sa) or None),
                                       ctypes.byref(eof), _ptr(counts), int(device), ctypes.c_void_p(int(stream) or None)))
    return int(eof.value), counts


def lcp_from_text(text, device=0):
    """fmx_lcp_from_text: the LCP array of reverse(text) + sentinel in the reference's convention (Util.bwtFm2LCP,
    util.scala:153-212; LCPCreator, bwtmerger.scala:558-652): entry r is the longest common prefix of the suffixes of rows
    r and r + 1, the last entry 0.  Suffix sort and LCP run on the device.  Returns uint32[len + 1]."""
    L = _lib.load()
    t = _text_array(text)
    lcp = np.zeros(t.size + 1, dtype=np.uint32)
    _lib.check(L.fmx_lcp_from_text(_ptr(t), t.size, _ptr(lcp), int(device)))
    return lcp


def lcp_from_text_dev(d_text, length, d_sa, d_lcp, device=0, stream=0):
    """fmx_lcp_from_text_dev: device pointers -- text[length] and the suffix array bwt_from_text_dev left in d_sa
    (u32[length + 1]) in, the LCP array (u32[length + 1]) out.  Allocates 5 (length + 1) bytes and synchronises `stream`."""
    L = _lib.load()
    _lib.check(L.fmx_lcp_from_text_dev(ctypes.c_void_p(int(d_text) or None), int(length), ctypes.c_void_p(int(d_sa) or None),
                                       ctypes.c_void_p(int(d_lcp) or None), int(device), ctypes.c_void_p(int(stream) or None)))


def lcp_last_phases():
    """fmx_lcp_last_phases: device ms of this thread's last lcp_from_text[_dev] in its three phases (successor array,
    text-order pass, gather)."""
    L = _lib.load()
    a, b, c = ctypes.c_double(), ctypes.c_double(), ctypes.c_double()
    _lib.check(L.fmx_lcp_last_phases(ctypes.byref(a), ctypes.byref(b), ctypes.byref(c)))
    return float(a.value), float(b.value), float(c.value)


def write_bwt(bwt_path, aux_path, bwt, eof, counts, bigEndian=True):
    """fmx_write_bwt: X.bwt (int64 size, int64 eof, the bytes; BWTLoader) and X.aux (256 int64; AUXLoader)."""
    L = _lib.load()
    b = np.ascontiguousarray(bwt, dtype=np.uint8).reshape(-1)
    c = np.ascontiguousarray(counts, dtype=np.int64).reshape(-1)
    if c.size != 256:
        raise ValueError("counts must have 256 entries")
    _lib.check(L.fmx_write_bwt(str(bwt_path).encode(), str(aux_path).encode(), _ptr(b), b.size, int(eof), _ptr(c),
                               1 if bigEndian else 0))
