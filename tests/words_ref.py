"""The context filter and whole-word search in plain Python: the checker the words tests rest on (include/fmx.h,
fmx_context_filter, fmx_search_context_batch).

SuffixRef holds a naive suffix array of s = reverse(text) + sentinel and answers, row by row, with the header's definitions:
the interval of a string, the byte behind a row's occurrence (text[pos + len], 0 at the text's end -- which the class also
checks to be the BWT byte of the row), LF^j(0), the filter's runs and the context search's ranges.  word_starts and
literal_word_starts are the end-to-end checkers: Python's re (fullmatch of every candidate span) and bytes.find with explicit
neighbour tests on the text, no lookaround."""
import re

import numpy as np

WORD_BYTES = bytes(sorted(set(b"0123456789ABCDEFGHIJKLMNOPQRSTUVWXYZabcdefghijklmnopqrstuvwxyz_") | set(range(0x80, 0x100))))
BOUNDARY = bytes(c for c in range(256) if c not in set(WORD_BYTES))
CTX_START = 0x80


def naive_suffix_array(s):
    return sorted(range(len(s)), key=lambda i: s[i:])


def doubling_suffix_array(s):
    """The same array by prefix doubling (numpy), for texts the naive sort is too slow for; tests/test_words_cpu.py holds it to
    the naive one."""
    n = len(s)
    rank = np.frombuffer(bytes(s), dtype=np.uint8).astype(np.int64)
    k = 1
    while True:
        nxt = np.full(n, -1, dtype=np.int64)
        if k < n:
            nxt[: n - k] = rank[k:]
        key = rank * (max(n, 256) + 2) + (nxt + 1)
        order = np.argsort(key, kind="stable")
        sk = key[order]
        new = np.zeros(n, dtype=np.int64)
        new[order] = np.concatenate([[0], np.cumsum(sk[1:] != sk[:-1])])
        rank = new
        if int(rank.max()) == n - 1:
            return order.tolist()
        k *= 2


class SuffixRef:
    def __init__(self, text):
        self.text = bytes(text)
        assert 0 not in self.text
        self.s = self.text[::-1] + b"\0"
        self.n = len(self.s)
        self.sa = naive_suffix_array(self.s) if self.n <= 4096 else doubling_suffix_array(self.s)
        # BWT of s: the byte in front of each suffix, the sentinel row's read as 0
        self.bwt = bytes(self.s[i - 1] if i else 0 for i in self.sa)
        self.eof = self.sa.index(0)
        self.isa = [0] * self.n
        self._iv = {}
        for r, i in enumerate(self.sa):
            self.isa[i] = r

    def interval(self, x):
        """[sp, ep) of the TEXT string x: the rows whose suffix of s begins with reverse(x)."""
        p = bytes(x)[::-1]
        if p not in self._iv:
            rows = [r for r in range(self.n) if self.s[self.sa[r]:self.sa[r] + len(p)] == p]
            assert rows == list(range(rows[0], rows[-1] + 1)) if rows else True
            self._iv[p] = (rows[0], rows[-1] + 1) if rows else (0, 0)
        return self._iv[p]

    def pos(self, r, length):
        return self.n - 1 - length - self.sa[r]

    def behind(self, r, length):
        """The text byte behind the occurrence of a string of `length` bytes at row r; 0 where the text ends."""
        p = self.pos(r, length) + length
        b = self.text[p] if p < len(self.text) else 0
        assert b == self.bwt[r]
        return b

    def lf_chain(self, j):
        """LF^j(0): the row with SA == n - 1 - j."""
        return self.isa[self.n - 1 - j]

    def filter(self, records, right, modes=None):
        """records [(group, len, sp, ep)] -> (off, runs [(group, len - lead, run_sp, run_ep)]) by the header's rules."""
        right = set(bytes(right))
        off, out = [0], []
        for j, (g, ln, sp, ep) in enumerate(records):
            md = modes[j] if modes is not None else 0
            lead = md & 127
            cand = []
            if ln > lead and sp < ep:
                if md & CTX_START:
                    if sp < self.n and ln <= self.n - 1 and self.lf_chain(ln) == sp:
                        cand = [sp]
                else:
                    cand = list(range(sp, min(ep, self.n)))
            passing = [r for r in cand if self.bwt[r] in right]
            for r in passing:
                if out and len(out) > off[-1] and out[-1][3] == r:
                    out[-1] = (g, ln - lead, out[-1][2], r + 1)
                else:
                    out.append((g, ln - lead, r, r + 1))
            off.append(len(out))
        return off, out

    def context_rows(self, x, left, right):
        """The rows of the TEXT string x whose neighbours are in the classes (0: an end of the text), ascending."""
        left, right = set(bytes(left)), set(bytes(right))
        x = bytes(x)
        sp, ep = self.interval(x)
        rows = []
        for r in range(sp, ep):
            p = self.pos(r, len(x))
            a = self.text[p - 1] if p > 0 else 0
            if a in left and self.behind(r, len(x)) in right:
                rows.append(r)
        return rows


def word_starts(text, regex, word=WORD_BYTES, max_len=16):
    """[(start, length)] of the matches of the bytes regex in text whose neighbours are no word bytes (or an end of the text):
    every match at every start, every length up to max_len a start allows (each end is tried with fullmatch)."""
    text = bytes(text)
    word = set(bytes(word))
    rx = re.compile(regex if isinstance(regex, bytes) else regex.encode("latin-1"), re.DOTALL)
    out = []
    for a in range(len(text)):
        if a > 0 and text[a - 1] in word:
            continue
        for b in range(a + 1, min(len(text), a + max_len) + 1):
            if b < len(text) and text[b] in word:
                continue
            if rx.fullmatch(text, a, b):
                out.append((a, b - a))
    return out


def literal_word_starts(text, q, word=WORD_BYTES):
    """Sorted starts of the whole-word occurrences of the bytes q (overlapping ones included)."""
    text, q = bytes(text), bytes(q)
    word = set(bytes(word))
    out, i = [], text.find(q)
    while i >= 0:
        j = i + len(q)
        if (i == 0 or text[i - 1] not in word) and (j == len(text) or text[j] not in word):
            out.append(i)
        i = text.find(q, i + 1)
    return out


def disjoint(hits):
    """The leftmost non-overlapping reading of [(start, length)]: at every start the longest, then left to right."""
    best = {}
    for a, ln in hits:
        best[a] = max(best.get(a, 0), ln)
    out, end = [], 0
    for a in sorted(best):
        if a >= end:
            out.append((a, best[a]))
            end = a + best[a]
    return out


def longest(hits):
    best = {}
    for a, ln in hits:
        best[a] = max(best.get(a, 0), ln)
    return sorted(best.items())
