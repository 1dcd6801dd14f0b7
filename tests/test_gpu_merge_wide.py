"""Append to an index of more than 2^32 rows, in both layouts: the rank walk's WIDE instantiations start only when
n > 2^32, and below this size no gap rank and no output row of 2^32 or more ever passed through k_mrg_walk, k_mrg_place and
k_mrg_emit.  The pattern of tests/test_gpu_extract_wide.py.

A is that file's text, 'b' x p + 'a' x q with p = 2^29 + 77 and q = 2^32 + 1000 (n = p + q + 1 rows): s_A = a^q b^p $, its
rows are $; a^k b^p $ for k = q .. 1; b^k $ for k = 1 .. p; the BWT is 'b', filler (eof = 1), 'a' x (q - 1), 'b' x (p - 1),
'a'.  B is a short text over {a, b, c} that begins with 'c' and holds "ab" and "ba"; R = reverse(B) ends with 'c'.

The closed-form rule.  A new suffix is X = u . s_A with u = R[j..], which ends with 'c'.  Write u = a^i b^m z with z
beginning with 'a' or 'c' (i and m may be 0; i <= q and m < p).  The rows of A below X are
    the row of $ ................................ 1
    rows a^k b^p $ ............................... q when i = 0; else the q - i with k > i, and the one with k = i iff z
                                                   begins with 'c' (b^p against b^m z: 'b' against z's first byte)
    rows b^k $ ................................... 0 when i > 0; else m (k <= m: $ is below z), or all p when z begins with 'c'
r_j is their sum.  The new suffixes' order among themselves is the order of u . a^(b + 1) (q is longer than any comparison).
New suffix of kept rank t stands in row r_j + t with byte R[j - 1]; j = 0 is the new eof row and takes the byte of the row
above; A's eof row (row 1) takes R's last byte 'c'; every other row of A keeps its byte.  The ranks of the u that begin with
'b' or 'c' are above 2^32 and come from occ on a wide handle; so are their output rows.  The rule is held to a brute-force
suffix sort at small p and q in the CPU case below; nothing of the library produces an expectation.

Seconds on the MI355X: the fixture (the BWT, both handles, the output buffer: 14 GB) takes 0.2 s when the module
runs alone and 5.8 s inside the whole suite, where its allocations meet memory other modules have just released; a layout's
three appends with their checks take 0.2 s (6 - 8 ms each in the piece, 2.7 ms in order and emit of 4.8 G rows).  SLOWEST_S is the fixture inside the suite; the limit of a test is three
times that, the margin tests/test_gpu_search_forms.py takes for the machine's load.
"""
import gc
import time

import numpy as np
import pytest

import findex_amd
from helpers import ends_at_a_fault

SLOWEST_S = 6
pytestmark = [pytest.mark.gpu, pytest.mark.timeout(3 * SLOWEST_S)]

LINE = 1 << 32
P = (1 << 29) + 77
Q = LINE + 1000
N = P + Q + 1
LAYOUTS = ("onehot", "bytes")
TEXTS = (b"cabbacab", b"cbaabcbbbaac")


def gap_rank(u, p, q):
    """rows of A below u . a^q b^p $, by the header's rule"""
    i = len(u) - len(u.lstrip(b"a"))
    rest = u[i:]
    m = len(rest) - len(rest.lstrip(b"b"))
    z = rest[m:]
    assert z[:1] in (b"a", b"c") and i <= q and m < p
    zc = z[:1] == b"c"
    below_a = q if i == 0 else q - i + (1 if zc else 0)
    below_b = 0 if i > 0 else (p if zc else m)
    return 1 + below_a + below_b


def merged_rule(p, q, B):
    """-> (rows of the new suffixes ascending, their bytes with 0 at the new eof row, the new eof row)"""
    R = B[::-1]
    b = len(B)
    order = sorted(range(b), key=lambda j: R[j:] + b"a" * (b + 1))
    rows = [gap_rank(R[j:], p, q) + t for t, j in enumerate(order)]
    assert rows == sorted(rows)
    byts = [R[j - 1] if j else 0 for j in order]
    return rows, byts, rows[order.index(0)]


def merged_bwt_small(p, q, B):
    """the whole merged BWT by the rule, on the host"""
    old = np.full(p + q + 1, ord("a"), dtype=np.uint8)
    old[0] = ord("b")
    old[q + 1:q + p] = ord("b")
    old[1] = B[0]                                             # A's eof row: R's last byte
    rows, byts, eof = merged_rule(p, q, B)
    out = np.zeros(p + q + 1 + len(B), dtype=np.uint8)
    new = np.zeros(out.size, dtype=bool)
    new[rows] = True
    out[~new] = old
    out[rows] = byts
    out[eof] = out[eof - 1]
    return out, eof


def test_rule_against_a_suffix_sort():
    from helpers import bwt_of_text
    for B in TEXTS + (b"c", b"cab", b"cba", b"ccabab", b"caabbaabbc"):
        for p, q in ((len(B) + 1, len(B) + 1), (len(B) + 3, len(B) + 9), (2 * len(B), len(B) + 2)):
            want, weof, _ = bwt_of_text((b"b" * p + b"a" * q + B)[::-1])
            got, eof = merged_bwt_small(p, q, B)
            assert eof == weof and np.array_equal(got, want), (B, p, q)


class Wide:
    pass


@pytest.fixture(scope="module")
def wide():
    import torch
    w = Wide()
    t0 = time.time()
    gc.collect()
    torch.cuda.empty_cache()
    bwt = torch.full((N,), ord("a"), dtype=torch.uint8, device="cuda")
    bwt[0] = ord("b")
    bwt[Q + 1:Q + P] = ord("b")
    counts = np.zeros(256, dtype=np.int64)
    counts[ord("a")], counts[ord("b")] = Q, P
    torch.cuda.synchronize()
    w.hip = {}
    try:
        for layout in LAYOUTS:
            findex_amd.set_layout(layout)
            w.hip[layout] = findex_amd.HipFMSearcher.from_device(bwt.data_ptr(), N, 1, counts)
    finally:
        findex_amd.set_layout("auto")
    bwt[1] = ord("c")                                         # what A's rows hold after an append of a B that begins with 'c'
    w.old = bwt
    w.out = torch.empty(N + max(len(B) for B in TEXTS) + 64, dtype=torch.uint8, device="cuda")
    for layout in LAYOUTS:
        assert w.hip[layout].stats()["layout"] == (0 if layout == "onehot" else 1) and w.hip[layout].n == N > LINE
    print("wide merge: index of %d rows in both layouts, %.1f s" % (N, time.time() - t0))
    yield w
    for h in w.hip.values():
        h.close()
    del w.old, w.out
    gc.collect()
    torch.cuda.empty_cache()


@pytest.mark.parametrize("layout", LAYOUTS)
@ends_at_a_fault
def test_append_above_two_to_the_32(wide, layout):
    import torch
    hip = wide.hip[layout]
    for B, opts in ((TEXTS[0], {}), (TEXTS[1], {}), (TEXTS[1], {"segment": 2, "warmup": 1})):
        b = len(B)
        rows, byts, eof_row = merged_rule(P, Q, B)
        assert min(rows) > LINE and len(set(gap_rank(B[::-1][j:], P, Q) for j in range(b))) >= 3      # every output row and rank lies above 2^32
        text = torch.from_numpy(np.frombuffer(B, dtype=np.uint8).copy()).cuda()
        wide.out.fill_(0xA5)
        torch.cuda.synchronize()
        t0 = time.time()
        eof, counts = hip.append_text_dev(text.data_ptr(), b, wide.out.data_ptr(), stream=torch.cuda.current_stream().cuda_stream, **opts)
        st = hip.merge_last()
        print("%s %r %s: %.2f s; piece %.1f walk %.2f fix-up %.2f emit %.1f ms; %d walk, %d fix-up steps" % (
            layout, B, opts, time.time() - t0, st["piece_ms"], st["walk_ms"], st["fixup_ms"], st["emit_ms"], st["walk_steps"], st["fixup_steps"]))
        assert eof == eof_row
        want_counts = np.zeros(256, dtype=np.int64)
        want_counts[ord("a")], want_counts[ord("b")] = Q, P
        want_counts += np.bincount(np.frombuffer(B, dtype=np.uint8), minlength=256)
        assert np.array_equal(counts, want_counts)
        assert bool((wide.out[N + b:] == 0xA5).all().item())
        # the rows of A between the new suffixes, slice against slice; the new rows themselves
        got_new = wide.out[torch.tensor(rows, device="cuda")].cpu().numpy()
        want_new = np.array(byts, dtype=np.uint8)
        at = rows.index(eof_row)
        # the filler: the byte of the row above, a new suffix's or the row of A that stands there (`at` new rows lie before)
        want_new[at] = byts[at - 1] if at and rows[at - 1] == eof_row - 1 else int(wide.old[eof_row - 1 - at].item())
        assert np.array_equal(got_new, want_new), (got_new, want_new)
        prev_out, prev_old = 0, 0
        for t, r in enumerate(rows + [N + b]):
            ln = r - prev_out
            assert torch.equal(wide.out[prev_out:r], wide.old[prev_old:prev_old + ln]), (layout, B, t)
            prev_out, prev_old = r + 1, prev_old + ln
        assert prev_old == N
        if not opts:
            assert st["fixup_steps"] == 0 and st["walk_steps"] == b and st["rounds"] == 1 and st["context"] == 4096
        else:
            assert st["walk_steps"] > b
