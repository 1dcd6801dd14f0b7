"""Passages in plain Python: the checker the passages tests rest on (include/fmx.h, fmx_corpus_passages).  No library call.

Per hit the occurrences of corpus_ref.escape_bytes(term) in the file's slice of RefCorpus.stream come from a bytes.find loop
(overlaps included); every start is tried, the value of its window added up with Python floats in ascending slot order
(Python doubles do not fuse); raw_off / raw_len come from RefCorpus.table.  ignore_case: the find runs over the ASCII-lowered
slice with the lowered term.  words: an occurrence counts when the stream bytes next to it are no word bytes (words_ref) or the
file ends there -- the separator is no word byte, so this is the rule of the whole stream."""
import bisect

import corpus_ref
import words_ref

_WORD = set(words_ref.WORD_BYTES)


class PassagesRef:
    def __init__(self, ref):
        self.ref = ref
        self._occ = {}

    def occurrences(self, d, term, words=False, ignore_case=False):
        """(starts, length): the stream positions of the first bytes of the occurrences of `term` in file d, ascending."""
        key = (d, bytes(term), words, ignore_case)
        if key not in self._occ:
            lo, hi = self.ref.doc_start[d], self.ref.doc_start[d + 1] - 1          # without the separator
            hay, esc = self.ref.stream[lo:hi], corpus_ref.escape_bytes(bytes(term))
            find_in, needle = (hay.lower(), esc.lower()) if ignore_case else (hay, esc)
            out, i = [], find_in.find(needle)
            while i >= 0:
                j = i + len(esc)
                if not words or ((i == 0 or hay[i - 1] not in _WORD) and (j == len(hay) or hay[j] not in _WORD)):
                    out.append(lo + i)
                i = find_in.find(needle, i + 1)
            self._occ[key] = (out, len(esc))
        return self._occ[key]

    def passage(self, d, occ, lens, weights, window):
        """One hit from its slots' occurrence lists `occ` (starts) and lengths: ((raw_off, mask, value, raw_len, n_occ), tf)."""
        tf = [len(o) for o in occ]
        starts = sorted(set(f for o in occ for f in o))
        if not starts:
            return (0, 0, 0.0, 0, 0), tf
        best = None
        for a in starts:
            value, mask = 0.0, 0
            for s, (o, ln) in enumerate(zip(occ, lens)):
                # a slot's occurrences are ascending and of one length: the first f >= a ends first, so it decides for all
                x = bisect.bisect_left(o, a)
                if x < len(o) and o[x] + ln - 1 < a + window:
                    value = value + weights[s]
                    mask |= 1 << s
            if best is None or value > best[0]:
                best = (value, a, mask)
        value, a, mask = best
        b = min(a + window, self.ref.doc_start[d + 1] - 1)
        raw_off = self.ref.table[a][2]
        assert self.ref.table[a][0] == d and self.ref.table[b - 1][0] == d
        return (raw_off, mask, value, self.ref.table[b - 1][2] + 1 - raw_off, sum(tf)), tf

    def run(self, queries, hit_off, hit_doc, window, weights=None, words=False, ignore_case=False):
        """-> (records, tf rows padded with 0 to the longest query's slots), one per hit in the order of hit_doc."""
        stride = max([len(q) for q in queries] + [0])
        recs, rows, at = [], [], 0
        for i, q in enumerate(queries):
            ws = [1.0] * len(q) if weights is None else [float(w) for w in weights[at:at + len(q)]]
            at += len(q)
            for h in range(int(hit_off[i]), int(hit_off[i + 1])):
                d = int(hit_doc[h])
                found = [self.occurrences(d, t, words, ignore_case) for t in q]
                rec, tf = self.passage(d, [f[0] for f in found], [f[1] for f in found], ws, window)
                recs.append(rec)
                rows.append(tf + [0] * (stride - len(tf)))
        return recs, rows
