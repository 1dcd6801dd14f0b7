"""The yardstick of the LCP tests, written from the definition: with s = reverse(text) + sentinel and SA its suffix array,
LCP[r] = the longest common prefix of the suffixes of rows r and r + 1 for r < n - 1, LCP[n - 1] = 0 (a row is paired
with the row below it).  kasai() is linear on every input (the match length drops by at most one from a text position
to the next); brute() compares byte by byte and is for short strings only."""
import numpy as np


def s_of_text(text):
    """reverse(text) + the sentinel 0, as bytes."""
    return bytes(text)[::-1] + b"\0"


def kasai(s, sa):
    """s: bytes ending in its unique smallest symbol; sa: its suffix array.  Returns uint32[n]."""
    s = bytes(s)
    n = len(s)
    sa = np.asarray(sa, dtype=np.int64)
    assert sa.size == n
    isa = np.empty(n, dtype=np.int64)
    isa[sa] = np.arange(n)
    sal = sa.tolist()
    isal = isa.tolist()
    out = [0] * n
    h = 0
    for i in range(n):
        r = isal[i]
        if r == n - 1:
            h = 0
            continue
        j = sal[r + 1]
        while s[i + h] == s[j + h]:          # ends at the sentinel at the latest: it occurs once
            h += 1
        out[r] = h
        if h:
            h -= 1
    return np.array(out, dtype=np.uint32)


def brute(s, sa):
    s = bytes(s)
    n = len(s)
    out = np.zeros(n, dtype=np.uint32)
    for r in range(n - 1):
        a, b = int(sa[r]), int(sa[r + 1])
        h = 0
        while a + h < n and b + h < n and s[a + h] == s[b + h]:
            h += 1
        out[r] = h
    return out


def sorted_sa(s):
    """The suffix array by sorting the suffixes themselves (short strings)."""
    s = bytes(s)
    return np.array(sorted(range(len(s)), key=lambda i: s[i:]), dtype=np.int64)


def lcp_file_bytes(lcp):
    """X.lcp as LCPCreator writes it: entries 0 .. n - 2, big-endian int32, no header."""
    lcp = np.asarray(lcp)
    return lcp[: lcp.size - 1].astype(">u4").tobytes()
