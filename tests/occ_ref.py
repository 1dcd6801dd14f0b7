"""Three expectations for fmx_occurrences (include/fmx.h) in plain Python and numpy; none uses the library.

  from_records : the header's definitions applied one after the other to (group, len, sp, ep) records and a suffix array;
  brute_regex  : the Glushkov tables of oracle.retree simulated forwards over the text from every start -- no index at all;
  from_frontier: helpers.frontier_oracle's results (the oracle's getPrevRange, level by level) through from_records.

brute_regex against from_frontier says that pos = n - 1 - len - SA[row] is where the matched string stands, read in the
regex's own order."""
import numpy as np

import helpers

OCC = np.dtype([("group", np.uint32), ("len", np.uint32), ("pos", np.uint64), ("doc", np.uint32), ("raw_len", np.uint32),
                ("raw_off", np.uint64)])
WORDS = (b"ab", b"abc", b"cab", b"b", b"aab", b"\n", b" ", b"ca")
REGEXES = ("ab", "a+b", "a.b", "c(a|b)*c", "ab*", "[a-c]+", "b.*b")
MAX_LEN = 12

_made = {}


def word_text():
    """1500 words drawn by PCG64(3) from WORDS."""
    if "text" not in _made:
        rng = np.random.Generator(np.random.PCG64(3))
        _made["text"] = b"".join(WORDS[i] for i in rng.integers(0, len(WORDS), 1500).tolist())
    return _made["text"]


def suffix_array(T):
    """SA of s = reverse(T) + sentinel, as the index numbers its rows (naive sort: small texts)."""
    s = bytes(T)[::-1] + b"\0"
    return np.array(sorted(range(len(s)), key=lambda i: s[i:]), dtype=np.int64)


def oracle_index(T):
    """(the oracle's searcher over the index of T, its suffix array), made once per text."""
    T = bytes(T)
    if T not in _made:
        import oracle
        _made[T] = (oracle.NaiveFMSearcher.from_mem(*helpers.bwt_of_text(T[::-1])), suffix_array(T))
    return _made[T]


def reduce_pairs(pairs, mode):
    """One group's (pos, len) pairs by the mode: sorted distinct pairs, the longest at each pos, the leftmost disjoint ones."""
    out = sorted(set(pairs))
    if mode == "all":
        return out
    longest = {}
    for p, ln in out:
        longest[p] = max(ln, longest.get(p, 0))
    out = sorted(longest.items())
    if mode == "longest":
        return out
    assert mode == "disjoint"
    taken, end = [], 0
    for p, ln in out:
        if p >= end:
            taken.append((p, ln))
            end = p + ln
    return taken


def as_csr(per_group, docs=None):
    """[[(pos, len)] per group] -> (off, OCC array); docs: a corpus_ref.RefCorpus whose stream the text is."""
    off = np.zeros(len(per_group) + 1, dtype=np.uint64)
    off[1:] = np.cumsum([len(g) for g in per_group])
    occ = np.zeros(int(off[-1]), dtype=OCC)
    i = 0
    for g, pairs in enumerate(per_group):
        for p, ln in pairs:
            if docs is None:
                occ[i] = (g, ln, p, 0xFFFFFFFF, ln, p)
            else:
                d, _, ro = docs.table[p]
                occ[i] = (g, ln, p, d, docs.table[p + ln - 1][2] + 1 - ro, ro)
            i += 1
    return off, occ


def from_records(T, sa, records, mode, max_per=None, docs=None, n_groups=None):
    """records: (group, len, sp, ep) tuples.  -> (off[n_groups + 1], OCC array)."""
    m = len(T)
    if n_groups is None:
        n_groups = max([r[0] for r in records], default=0) + 1
    per_group = [[] for _ in range(n_groups)]
    for g, ln, sp, ep in records:
        g, ln, sp, ep = int(g), int(ln), int(sp), int(ep)
        if ep <= sp or ln == 0:
            continue
        take = ep - sp if not max_per else min(ep - sp, max_per)
        for r in range(sp, sp + take):
            if sa[r] + ln > m:
                continue
            pos = m - ln - int(sa[r])
            if docs is not None and pos + ln > docs.doc_start[docs.table[pos][0] + 1] - 1:
                continue
            per_group[g].append((pos, ln))
    return as_csr([reduce_pairs(p, mode) for p in per_group], docs)


def brute_regex(tables, T, max_len):
    """[(pos, len)] of every match of one regex (ReTree.tables()) of at most max_len bytes, by simulating the states forwards
    from every start.  The reference's rule: a state that isLast emits and is NOT expanded (so "ab*" matches only "a")."""
    T = bytes(T)
    c, last, follows = tables["c"], tables["isLast"], tables["follows"]
    out = set()
    for p in range(len(T)):
        active = list(tables["firsts"])
        ln = 0
        while active and p + ln < len(T) and ln < max_len:
            ch = T[p + ln]
            ln += 1
            nxt = []
            for s in active:
                if c[s] != ch:
                    continue
                if last[s]:
                    out.add((p, ln))
                else:
                    nxt += follows[s]
            active = list(set(nxt))              # multiplicity does not matter to the set of matches
    return sorted(out)


def brute_csr(tables_list, T, max_len, mode, docs=None):
    """brute_regex for a batch, reduced by the mode; docs: matches that do not lie inside one document go first."""
    def inside(p, ln):
        return docs is None or p + ln <= docs.doc_start[docs.table[p][0] + 1] - 1
    return as_csr([reduce_pairs([x for x in brute_regex(t, T, max_len) if inside(*x)], mode) for t in tables_list], docs)


def from_frontier(orc, tables_list, sa, T, max_len, mode, max_per=None):
    """The oracle's frontier results for a batch of regexes through from_records."""
    res, _, _ = helpers.frontier_oracle(orc, tables_list, max_len)
    return from_records(T, sa, res.tolist(), mode, max_per, n_groups=len(tables_list))


def regex_tables(regexes=REGEXES):
    from oracle import retree as R
    return [R.ReTree(R.re2post(r)).tables() for r in regexes]
