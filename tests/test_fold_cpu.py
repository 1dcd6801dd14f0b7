"""Case folding without a device: the three references of tests/fold_ref.py against one another, the identity
map against the oracle's exact search, the header's struct under a strict C compile, every refusal the calls decide from their
arguments alone, fold_regex against Python's re through the oracle's own regex engine, and the command-line parsers."""
import ctypes
import os
import re
import shutil
import subprocess

import numpy as np
import pytest

import approx_ref
import fold_ref
import oracle
from conftest import TESTDATA
from findex_amd import ASCII_FOLD, _lib, check_fold, fold_map
from findex_amd.regex import fold_regex
from helpers import lf_walk_patterns, pack_patterns, synth_bwt
from oracle import engines as E
from oracle import retree as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ARG = 3


def spellings(p):
    return [p, p.lower(), p.upper(), p.swapcase()]


@pytest.fixture(scope="module")
def mixed_text():
    with open(os.path.join(TESTDATA, "test3072.txt"), "rb") as f:
        return fold_ref.mixed_case(f.read())


# ---------------------------------------------------------------- the references
def test_maps():
    assert ASCII_FOLD == fold_ref.ASCII and len(ASCII_FOLD) == 256
    assert fold_map([b"aA", (0x62, 0x42)])[0x61] == 0x41 and fold_map([])[:] == fold_ref.IDENTITY
    assert fold_map([b"ab", b"bc"]) == fold_ref.make_map([b"abc"])                    # classes that share a member merge
    assert fold_map([(b"a", b"A")]) == fold_map([b"aA"])
    for bad in ([b"a\0"], [bytes(range(1, 10))]):
        with pytest.raises(ValueError):
            fold_map(bad)
    swapped = bytearray(range(256))
    swapped[0x61], swapped[0x41] = 0x41, 0x61                                         # a -> A -> a: not idempotent
    for bad in (bytes(swapped), bytes([1]) + bytes(range(1, 256)), bytes(255)):
        with pytest.raises(ValueError):
            check_fold(bad)


def test_references_agree_on_the_mixed_case_text(mixed_text):
    s = mixed_text
    assert sum(1 for c in s if 65 <= c <= 90) > 800                                   # the golden text has no capitals of its own
    orc = approx_ref.index_of(s)[0]
    rng = np.random.default_rng(280)
    pats = [b"", b"#", b"q#", b"\0", s[-2:] + b"\0"]
    for m in range(25):
        at = int(rng.integers(0, len(s) - m + 1))
        pats += spellings(s[at:at + m])
    several = 0
    for p in pats:
        w = fold_ref.window_hits(s, p, ASCII_FOLD)
        hits, steps, depth = fold_ref.walk(orc, p, ASCII_FOLD)
        assert w == fold_ref.dfs_hits(orc, p, ASCII_FOLD) == hits, p
        assert depth <= len(p)                                                        # a class of two pushes one sibling per byte at most
        several += len(w) >= 2
    assert several >= 4                                                               # a string of one byte, in its four spellings


def test_references_agree_where_every_variant_occurs():
    s = bytes(np.random.default_rng(282).choice([97, 65], 4096).astype(np.uint8))
    orc = approx_ref.index_of(s)[0]
    for p in (b"a", b"aA", b"a" * 5, b"A" * 10, b"a" * 14):
        w = fold_ref.window_hits(s, p, ASCII_FOLD)
        hits, steps, depth = fold_ref.walk(orc, p, ASCII_FOLD)
        assert w == fold_ref.dfs_hits(orc, p, ASCII_FOLD) == hits
        assert len(w) == 2 ** len(p) if len(p) <= 5 else len(w) > 900
        assert depth >= len(p) - 2                                                    # a sibling waits at nearly every level
        assert steps >= 2 * len(w) - 2                                                # every edge of the trie of variants is a step


def test_references_agree_on_a_synthetic_bwt():
    """No text stands behind these rows: the definition rests on cf / occ alone."""
    fold = fold_ref.make_map([range(97, 105), (105, 106), (120, 121, 122)])
    for n, eof in ((449, 0), (128, 64), (4500, 4499)):
        orc = oracle.NaiveFMSearcher.from_mem(*synth_bwt(n, 97, 112, seed=n, eof=eof))
        rng = np.random.default_rng(n)
        pats = [p for m in (1, 2, 4, 7) for p in lf_walk_patterns(orc, rng, 10, m, 0.3, alphabet=list(range(97, 113)))]
        pats += [b"", b"z", b"xa", bytes([0]), b"a" + bytes([0])]
        total = 0
        for p in pats:
            hits, steps, _ = fold_ref.walk(orc, p, fold)
            assert hits == fold_ref.dfs_hits(orc, p, fold), (n, eof, p)
            total += len(hits)
        assert total > 100


def test_identity_map_is_the_oracles_exact_search(mixed_text):
    orc = approx_ref.index_of(mixed_text)[0]
    rng = np.random.default_rng(286)
    pats = [b"", b"#", b"\0", mixed_text[:40], mixed_text[-9:] + b"\0"]
    for m in (1, 3, 8, 20):
        for at in rng.integers(0, 3000, 6).tolist():
            pats += [mixed_text[at:at + m], mixed_text[at:at + m].swapcase()]
    buf, off = pack_patterns(pats)
    sp, ep, steps = orc.search_batch(buf, off)
    for j, p in enumerate(pats):
        hits, st, depth = fold_ref.walk(orc, p, fold_ref.IDENTITY)
        assert hits == ([(int(sp[j]), int(ep[j]))] if sp[j] < ep[j] else []), p
        assert st == int(steps[j]) and depth == 0, p
        # a lead that covers the whole pattern makes every step exact, whatever the map says
        assert fold_ref.walk(orc, p, ASCII_FOLD, lead=len(p))[:2] == (hits, st), p


# ---------------------------------------------------------------- the header
def test_abi_and_struct_sizes():
    assert _lib.load().fmx_abi_version() == 5
    assert ctypes.sizeof(_lib.fmx_stats_t) == 232
    assert ctypes.sizeof(_lib.fmx_fold_opts) == 264 and _lib.fmx_fold_opts.flags.offset == 256
    assert _lib.FMX_FOLD_MAX_CLASS == 8 and _lib.FMX_FOLD_MAX_LEN == 255


@pytest.mark.skipif(shutil.which("gcc") is None, reason="needs gcc")
def test_struct_layout_against_a_strict_c_compile(tmp_path):
    src = tmp_path / "sizes.c"
    src.write_text(
        "#include <stddef.h>\n#include <stdio.h>\n#include <fmx.h>\n"
        "int main(void) {\n"
        "  printf(\"%d %d %d %d %d %d\\n\", (int)sizeof(fmx_fold_opts), (int)offsetof(fmx_fold_opts, flags),\n"
        "         (int)offsetof(fmx_fold_opts, reserved), FMX_FOLD_MAX_CLASS, FMX_FOLD_MAX_LEN, FMX_ABI_VERSION);\n"
        "  return 0;\n}\n")
    exe = tmp_path / "sizes"
    subprocess.check_call(["gcc", "-std=c99", "-Wall", "-Wextra", "-Werror", "-pedantic", "-I" + os.path.join(ROOT, "include"),
                           str(src), "-o", str(exe)])
    out = subprocess.run([str(exe)], capture_output=True, text=True, timeout=60)
    assert out.stdout.split() == ["264", "256", "260", "8", "255", "5"]


# ---------------------------------------------------------------- refusals that need no device
def opts_of(fold=None, flags=0, reserved=0):
    o = _lib.fmx_fold_opts()
    ctypes.memmove(o.fold, bytes(fold if fold is not None else ASCII_FOLD), 256)
    o.flags, o.reserved = flags, reserved
    return o


def bad_maps():
    swapped = bytearray(range(256))
    swapped[0x61], swapped[0x41] = 0x41, 0x61
    to_zero = bytearray(range(256))
    to_zero[0x61] = 0
    zero_moved = bytearray(range(256))
    zero_moved[0] = 5
    nine = bytearray(range(256))
    for c in range(0x61, 0x6A):
        nine[c] = 0x61
    return [(bytes(swapped), b"idempotent"), (bytes(to_zero), b"folds to 0"), (bytes(zero_moved), b"folds to"), (bytes(nine), b"more than 8")]


def test_argument_refusals_before_any_device():
    """Everything the calls decide from their arguments alone comes before the handle is looked at, and the null handle is
    refused last with a message of its own: on a machine without a GPU each refusal still shows by its message."""
    L = _lib.load()
    n_out = ctypes.c_size_t(77)
    pat = np.frombuffer(b"abcd", dtype=np.uint8)
    off = np.array([0, 2, 4], dtype=np.uint64)
    out_off = np.zeros(3, dtype=np.uint64)
    out = np.zeros(4, dtype=[("regex", np.uint32), ("len", np.uint32), ("sp", np.uint64), ("ep", np.uint64)])

    def host(h=None, p=pat, o=off, k=2, opts=None, cap=4, n=n_out, oo=out_off):
        return L.fmx_search_fold_batch(h, p.ctypes.data, o.ctypes.data, k, ctypes.byref(opts) if opts is not None else None,
                                       oo.ctypes.data if oo is not None else None, out.ctypes.data, cap,
                                       ctypes.byref(n) if n is not None else None)

    def dev(h=None, k=2, opts=None, cap=4, n=n_out):
        return L.fmx_search_fold_batch_dev(h, pat.ctypes.data, off.ctypes.data, k, ctypes.byref(opts) if opts is not None else None,
                                           out_off.ctypes.data, out.ctypes.data, cap, ctypes.byref(n) if n is not None else None, None)

    cases = [(dict(), b"handle"), (dict(n=None), b"n_out"), (dict(opts=opts_of(flags=1)), b"must be 0"),
             (dict(opts=opts_of(reserved=9)), b"must be 0"), (dict(k=(1 << 26) + 1), b"2^26"), (dict(cap=1 << 32), b"2^32")]
    cases += [(dict(opts=opts_of(m)), word) for m, word in bad_maps()]
    for form in (host, dev):
        for kw, word in cases:
            assert form(**kw) == ARG, (form.__name__, kw)
            assert word in L.fmx_last_error(), (form.__name__, kw, L.fmx_last_error())
        assert form(opts=opts_of()) == ARG and b"handle" in L.fmx_last_error()         # a valid map passes on to the handle
    assert host(o=np.array([0, 3, 2], dtype=np.uint64)) == ARG and b"non-decreasing" in L.fmx_last_error()
    assert host(oo=None) == ARG and b"null argument" in L.fmx_last_error()
    long_pat = np.full(300, 97, dtype=np.uint8)
    assert host(p=long_pat, o=np.array([0, 255, 256], dtype=np.uint64)) == ARG and b"handle" in L.fmx_last_error()      # 255 bytes pass
    assert host(p=long_pat, o=np.array([0, 256, 300], dtype=np.uint64)) == ARG and b"255 bytes" in L.fmx_last_error()
    assert n_out.value == 77                                 # a refused call writes nothing
    a, b = ctypes.c_double(-1), ctypes.c_double(-1)
    c, d = ctypes.c_uint64(5), ctypes.c_uint64(5)
    assert L.fmx_fold_last(ctypes.byref(a), ctypes.byref(b), ctypes.byref(c), ctypes.byref(d)) == 0
    assert a.value >= 0 and b.value >= 0
    assert L.fmx_fold_last(None, None, None, None) == 0


def test_context_fold_refusals_need_no_device():
    L = _lib.load()
    vp = ctypes.c_void_p
    fake = ctypes.create_string_buffer(8192)
    i = ctypes.cast(fake, vp)

    def call(idx, pats, fold="ok", ctx="ok", flags=0, dev=False):
        pat = np.frombuffer(b"".join(pats), dtype=np.uint8)
        off = np.concatenate([[0], np.cumsum([len(p) for p in pats])]).astype(np.uint64)
        o = _lib.fmx_context_opts()
        o.flags = flags
        f = fold if fold != "ok" else opts_of()
        out_off = np.zeros(off.size, dtype=np.uint64)
        out = np.zeros(3, dtype=np.uint64)
        n = ctypes.c_size_t()
        args = [idx, pat.ctypes.data_as(vp), off.ctypes.data_as(vp), off.size - 1, ctypes.byref(o) if ctx == "ok" else None,
                ctypes.byref(f) if f is not None else None, out_off.ctypes.data_as(vp), out.ctypes.data_as(vp), 1, ctypes.byref(n)]
        rc = L.fmx_search_context_fold_batch_dev(*args, None) if dev else L.fmx_search_context_fold_batch(*args)
        return rc, L.fmx_last_error()

    for dev in (False, True):
        for m, word in bad_maps():
            rc, msg = call(i, [b"ab"], fold=opts_of(m), dev=dev)
            assert rc == ARG and word in msg, (word, msg)
        rc, msg = call(i, [b"ab"], fold=opts_of(flags=2), dev=dev)
        assert rc == ARG and b"must be 0" in msg
        rc, msg = call(i, [b"ab"], ctx=None, dev=dev)
        assert rc == ARG and b"opts" in msg
        rc, msg = call(i, [b"ab"], flags=1, dev=dev)
        assert rc == ARG and b"must be 0" in msg
        for fold in ("ok", None):                                                     # NULL: ASCII folding
            rc, msg = call(None, [b"ab"], fold=fold, dev=dev)
            assert rc == ARG and b"handle" in msg
    for pats, word in (([b"ab", b""], b"empty"), ([b"a\0b"], b"byte 0"), ([b"x" * 255], b"254")):
        rc, msg = call(i, pats)
        assert rc == ARG and word in msg, (word, msg)


# ---------------------------------------------------------------- fold_regex
REGEXES = [
    "the", "The", "THE", "t", "x_1", "café".encode().decode("latin-1"),                # literals
    "th.", ".he", "t.e", "a.", "\\.", "an\\.", "\\(he\\)", "a\\+", "x\\_1", "\\[",     # '.' and quotes
    "[ht]he", "[a-c]n", "[A-C]n", "[x-z]_", "t[g-i]e", "[_a]", "[X-c]", "[T-t]he", "[\\-a]n", "[a\\]]", "h[e3-5]",      # sets, intervals
    "(the|and)", "th(e|en)", "(a|x_)1?", "(t|T)he", "((a)n)d", "(he|the|then)", "(h|t)(e|h)",       # groups
    "a+", "an?", "a+n?d?", "the*n", "(an)+", "t?he", "h(el)*lo", "e+n+", "[ae]+", "(a|b)*n",       # * + ?
    "\\d", "x_\\d", "\\w\\w\\w\\w\\w", "e\\w",                                         # classes that stay as they are
    "[ab].", "[a-c]\\w", "[x-z]_\\d", "([ab]|c).", "[ht].\\w[n-p]\\d?",                        # a class or a dot AFTER a set
]
REFUSED = ["^the", "the$", "a{2}", "a}", "[^a]", "\\bthe", "\\n", "a\\1", "[\\d]", "[]", "[\\w-z]"]
TEXT = (b"The cat and THE Hat.\nthen an x_1 X_1 caf\xc3\xa9 CAF\xc3\xa9 hello HeLLo (he) a+ An. aNd [and] "
        b"tHe en ENNn a3 h4 _ - ] Tge tie b c C z_ Y_ bbn ABN x_9 x_8 hellllo eZ ez")


class OracleIndex:
    """What oracle.engines.nfa_matchSA reads of an index."""

    def __init__(self, orc):
        self.n, self.getPrevRange = orc.n, orc.getPrevRange


def re_strings(text, rx, flags, max_len):
    """The distinct strings of at most max_len bytes that rx matches somewhere in text (every start, every end)."""
    rx = re.compile(rx.encode("latin-1"), flags | re.DOTALL)
    return {text[a:b] for a in range(len(text)) for b in range(a + 1, min(len(text), a + max_len) + 1) if rx.fullmatch(text, a, b)}


def as_python(rx):
    """The regex as Python's re spells it: re2post's \\w is the interval A .. y and its \\d 0 .. 8 (IntervalPoint, `start until
    end`)."""
    return rx.replace("\\w", "[A-y]").replace("\\d", "[0-8]")


def test_fold_regex_is_pure_and_refuses_what_re_reads_differently():
    assert len(REGEXES) >= 40
    for rx in REGEXES:
        out = fold_regex(rx, ASCII_FOLD)
        assert out == fold_regex(rx, ASCII_FOLD) == fold_regex(rx.encode("latin-1"), ASCII_FOLD)
        assert "[" not in out.replace("\\[", "")                                        # no set is left for createNFA to refuse
        assert fold_regex(rx, fold_ref.IDENTITY).replace("(", "").replace(")", "") == rx.replace("(", "").replace(")", "") \
            or "[" in rx.replace("\\[", "")
    assert fold_regex("ab", ASCII_FOLD) == "(A|a)(B|b)" and fold_regex("a.\\d", ASCII_FOLD) == "(A|a).\\d" and fold_regex("\\w", ASCII_FOLD) == "(\\w|z)"
    assert fold_regex("[a-c]", ASCII_FOLD) == "(A|B|C|a|b|c)" and fold_regex("[wd]", ASCII_FOLD) == "(D|W|d|w)"
    assert fold_regex("a b", fold_map([b" x"])) == "a(\\ |x)b"
    for rx in REFUSED:
        with pytest.raises(ValueError):
            fold_regex(rx, ASCII_FOLD)
    with pytest.raises(ValueError):
        fold_regex("a", b"abc")
    # re2post's own syntax errors are left for the compiler
    for rx in ("[a", "[a-", "[c-a]"):
        assert fold_regex(rx, ASCII_FOLD).endswith(rx[1:])
        with pytest.raises(R.Re2PostSyntax):
            R.re2post(fold_regex(rx, ASCII_FOLD))


def test_fold_regex_against_python_re():
    """The oracle's NFA engine over reverse(TEXT), given the rewritten regex, finds the strings re finds in TEXT under
    re.IGNORECASE | re.ASCII -- and, as a check of the check, the plain regex finds re's without the flag."""
    orc = approx_ref.index_of(TEXT[::-1])[0]
    idx = OracleIndex(orc)
    max_len = 8

    def found(rx):
        out = set()
        for ln, sp, ep in E.nfa_matchSA(E.createNFA(R.re2post(rx)), idx, maxLength=max_len):
            out.add((ln, sp, ep))
        return out

    def want(strings):
        out = set()
        for x in strings:
            r = orc.search(x[::-1])
            assert r is not None
            out.add((len(x), int(r[0]), int(r[1])))
        return out

    more = 0
    for rx in REGEXES:
        folded = want(re_strings(TEXT, as_python(rx), re.IGNORECASE | re.ASCII, max_len))
        assert found(fold_regex(rx, ASCII_FOLD)) == folded, rx
        if "[" not in rx.replace("\\[", ""):                                          # (createNFA has no case for a set)
            exact = want(re_strings(TEXT, as_python(rx), 0, max_len))
            assert found(rx) == exact, rx
            more += len(folded) > len(exact)
    assert more >= 20


# ---------------------------------------------------------------- the command lines
def test_grep_cli_parses_i():
    from findex_amd import grep as cli
    a = cli.parser().parse_args(["base", "re", "-i", "-w", "-n"])
    assert a.ignore_case and a.words and a.line_number and cli.flags_of(a) == {"words": True, "ignore_case": True}
    assert cli.parser().parse_args(["base", "re", "--ignore-case"]).ignore_case
    d = cli.parser().parse_args(["base", "re"])
    assert d.ignore_case is False and cli.flags_of(d) == {} and not cli.by_lines(d)
    assert cli.flags_of(cli.parser().parse_args(["base", "re", "-i", "--and", "x"])) == {"ignore_case": True}
    assert "-i" in cli.parser().format_help()


def test_rank_cli_parses_i():
    from findex_amd import rank as cli
    assert cli.parser().parse_args(["base", "q", "-i"]).ignore_case and cli.parser().parse_args(["base", "q", "--ignore-case", "-w"]).words
    assert cli.parser().parse_args(["base", "q"]).ignore_case is False
    assert "--ignore-case" in cli.parser().format_help()
