"""Ranked retrieval in plain Python: the checker the ranking tests rest on (include/fmx.h, fmx_corpus_rank).

Per document the overlapping occurrences of corpus_ref.escape_bytes(term) in that document's slice of RefCorpus.stream are
counted with a bytes.find loop; df, len, avglen, the score by Python float arithmetic in the stated order (Python doubles do
not fuse), the candidate rule, and sorted(key=(-score, doc)).  The weights are an argument."""
import math

import corpus_ref


def count_overlapping(hay, needle):
    n, i = 0, hay.find(needle)
    while i >= 0:
        n += 1
        i = hay.find(needle, i + 1)
    return n


def default_weight(n_docs, df):
    return math.log(1.0 + (float(n_docs - df) + 0.5) / (float(df) + 0.5))


class RankRef:
    def __init__(self, ref):
        self.ref = ref
        self.n_docs = len(ref.docs)
        ds = ref.doc_start
        self.slices = [ref.stream[ds[d]:ds[d + 1] - 1] for d in range(self.n_docs)]        # without the separator
        self.raw_len = list(ref.raw_len)
        self.avglen = float(len(ref.stream) - self.n_docs - len(ref.esc_pos)) / float(self.n_docs)
        self._tf = {}

    def tf(self, term):
        """{doc: count} of the raw bytes `term`, counted in the escaped stream."""
        term = bytes(term)
        if term not in self._tf:
            esc = corpus_ref.escape_bytes(term)
            out = {}
            for d, s in enumerate(self.slices):
                c = count_overlapping(s, esc)
                if c:
                    out[d] = c
            self._tf[term] = out
        return self._tf[term]

    def postings(self, queries):
        """One {doc: tf} per term slot of `queries` (a list of lists of terms), in slot order."""
        return [self.tf(t) for q in queries for t in q]

    def weights(self, postings):
        return [default_weight(self.n_docs, len(p)) for p in postings]

    def score(self, d, tfs, ws, k1, b):
        """tfs / ws: the query's slots in ascending order."""
        r = 0.0 if self.avglen == 0 else float(self.raw_len[d]) / self.avglen
        nd = k1 * ((1.0 - b) + b * r)
        s = 0.0
        for tf, w in zip(tfs, ws):
            if tf > 0:
                s = s + w * ((float(tf) * (k1 + 1.0)) / (float(tf) + nd))
        return s

    def rank(self, q_sizes, postings, weights, top=10, k1=1.2, b=0.75, match="any"):
        """q_sizes: the slots per query.  -> (off, doc, score) as lists."""
        off, doc, score, at = [0], [], [], 0
        for m in q_sizes:
            post, ws = postings[at:at + m], weights[at:at + m]
            at += m
            cand = set()
            for p in post:
                cand |= set(p)
            if match == "all":
                cand = {d for d in cand if all(d in p for p in post)} if m else set()
            rows = [(self.score(d, [p.get(d, 0) for p in post], ws, k1, b), d) for d in cand]
            rows = sorted(rows, key=lambda r: (-r[0], r[1]))[:top]
            doc += [d for _, d in rows]
            score += [s for s, _ in rows]
            off.append(len(doc))
        return off, doc, score

    def rank_queries(self, queries, weights=None, **kw):
        post = self.postings(queries)
        ws = self.weights(post) if weights is None else list(weights)
        return self.rank([len(q) for q in queries], post, ws, **kw)
