"""String classes without a device: the three references of tests/classes_ref.py against one another on a
mixed-script text, on a text in which every variant occurs and on synthetic BWTs; all-literal patterns against the oracle's
exact search and a fold-map table against tests/fold_ref.py; the header's struct under a strict C compile; every refusal the
calls decide from their arguments alone, and their order; case_classes() against re.IGNORECASE; the tokeniser."""
import ctypes
import os
import re
import shutil
import subprocess

import numpy as np
import pytest

import approx_ref
import classes_ref as C
import fold_ref
import oracle
from findex_amd import _lib, unicode_fold
from helpers import lf_walk_patterns, pack_patterns, synth_bwt
from oracle import engines as E
from oracle import retree as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, "tests", "golden", "unicode_mixed.txt")
ARG = 3

# members of 1, 2, 3 and 4 bytes in one class; members that share a last byte and a two-byte suffix; classes of 1, 2, 9 and 16
SYNTH_TABLE = [
    [b"a", b"bc", b"def", b"ghij"],
    [b"kab", b"lab", b"mb", b"c"],
    [b"no"],
    [b"a", b"b"],
    [bytes([c]) for c in range(97, 106)],
    [bytes([c]) for c in range(97, 113)],
    [bytes([c]) for c in range(97, 109)] + [b"ma", b"mb", b"nab", b"opab"],
]


def golden_text():
    with open(GOLDEN, "rb") as f:
        return f.read()


def golden_patterns(text, rng, per_len=2, longest=24):
    """Text strings of 0 .. `longest` code points taken from the text, as they stand and in other spellings."""
    s = text.decode("utf-8")
    out = []
    for m in range(longest + 1):
        for _ in range(per_len):
            at = int(rng.integers(0, len(s) - m + 1))
            w = s[at:at + m]
            out += [w, w.lower(), w.upper(), w.swapcase()]
    out += ["Kelvin", "kelvin", "ſtop", "MISS", "σοφίασ", "IKI", "zebra", "ÜBER#"]
    # upper() and lower() may fold to several code points (ß): such a spelling is simply another query
    return [w.encode("utf-8") for w in out]


def synth_patterns(orc, rng, table, k, m):
    """Patterns that occur, by LF walk, with stretches that equal a member of a class replaced by the class."""
    out = []
    for p in lf_walk_patterns(orc, rng, k, m, 0.2, alphabet=list(range(97, 113))):
        row, j = [], 0
        while j < len(p):
            c = int(rng.integers(0, len(table)))
            fit = [mm for mm in table[c] if p.startswith(mm, j)]
            if fit and rng.random() < 0.6:
                row.append(256 + c)
                j += len(fit[0])
            else:
                row.append(p[j])
                j += 1
        out.append(row)
    return out


# ---------------------------------------------------------------- the references
def test_golden_text_holds_what_the_tests_need():
    s = golden_text().decode("utf-8")
    assert 4000 < len(golden_text()) < 8192
    for ch in "üÜéÉσςΣKſıIKÅÅ":
        assert ch in s, ch
    assert sum(1 for ch in s if len(ch.encode()) == 2) > 500 and sum(1 for ch in s if len(ch.encode()) == 3) > 20


def test_references_agree_on_the_mixed_script_text():
    text = golden_text()
    rev = text[::-1]
    orc = approx_ref.index_of(rev)[0]
    pats = golden_patterns(text, np.random.default_rng(300), per_len=1)
    el, off, cls_off, mem_off, mem_bytes = unicode_fold.class_table(pats)
    table = C.table_of(cls_off, mem_off, mem_bytes)
    assert max(len(m) for cl in table for m in cl) == 3 and any(len({len(m) for m in cl}) > 1 for cl in table)
    several = longer = 0
    for q, elements in zip(pats, C.unpack(el, off)):
        w = C.window_hits(rev, elements, table)
        hits, steps, depth = C.walk(orc, elements, table)
        assert w == C.dfs_hits(orc, elements, table) == hits, q
        assert depth <= 3 * len(elements)                                              # the largest class has 4 members
        several += len(w) >= 2
        longer += len({h[0] for h in w}) >= 2
    assert several >= 20 and longer >= 3                                               # spellings of different lengths of one query
    # what a user sees: the Kelvin sign meets k, the long s meets s, the final sigma meets the capital
    def find(q):
        t = unicode_fold.class_table([q.encode()])
        return C.window_hits(rev, C.unpack(t[0], t[1])[0], C.table_of(*t[2:]))

    assert len(find("kelvin")) == 4 and {h[0] for h in find("kelvin")} == {6, 8}
    assert len(find("miss")) == 3 and len(find("λόγοσ")) == 3 and not find("λογοσ")


def test_references_agree_where_every_variant_occurs():
    s = bytes(np.random.default_rng(282).choice([97, 65], 4096).astype(np.uint8))
    orc = approx_ref.index_of(s)[0]
    table, cid = C.fold_table(fold_ref.ASCII)
    for p in (b"a", b"aA", b"a" * 5, b"A" * 10):
        elements = C.folded(p, cid)
        w = C.window_hits(s, elements, table)
        hits, steps, depth = C.walk(orc, elements, table)
        assert w == C.dfs_hits(orc, elements, table) == hits
        assert [h[1:] for h in w] == fold_ref.dfs_hits(orc, p, fold_ref.ASCII)
        assert steps == fold_ref.walk(orc, p, fold_ref.ASCII)[1]                      # single bytes: the fold search's walk
        assert len(w) == 2 ** len(p) if len(p) <= 5 else len(w) > 900


def test_references_agree_on_synthetic_bwts():
    """No text stands behind these rows: the definition rests on cf / occ alone."""
    total = lens = 0
    for n, eof in ((449, 0), (128, 64), (4500, 4499)):
        orc = oracle.NaiveFMSearcher.from_mem(*synth_bwt(n, 97, 112, seed=n, eof=eof))
        rng = np.random.default_rng(n)
        pats = [p for m in (1, 2, 4, 7) for p in synth_patterns(orc, rng, SYNTH_TABLE, 10, m)]
        pats += [[], [122], [256], [261, 261], [0], [256, 0], [258, 257]]
        for elements in pats:
            hits, steps, depth = C.walk(orc, elements, SYNTH_TABLE)
            assert hits == C.dfs_hits(orc, elements, SYNTH_TABLE), (n, eof, elements)
            assert depth <= 15 * len(elements)
            total += len(hits)
            lens += len({h[0] for h in hits}) >= 2
    assert total > 300 and lens >= 10


def test_all_literal_patterns_are_the_oracles_exact_search():
    text = golden_text()
    orc = approx_ref.index_of(text[::-1])[0]
    rng = np.random.default_rng(301)
    pats = [b"", b"#", b"\0", text[:40][::-1], b"\0" + text[:5][::-1]]
    for m in (1, 3, 8, 20):
        for at in rng.integers(0, 4000, 6).tolist():
            pats += [text[at:at + m][::-1], text[at:at + m][::-1].swapcase()]
    buf, off = pack_patterns(pats)
    sp, ep, steps = orc.search_batch(buf, off)
    for j, p in enumerate(pats):
        hits, st, depth = C.walk(orc, C.literals(p), [])
        assert hits == ([(len(p), int(sp[j]), int(ep[j]))] if sp[j] < ep[j] else []), p
        assert st == int(steps[j]) and depth == 0, p


def test_fold_map_table_against_the_fold_reference():
    with open(os.path.join(ROOT, "tests", "golden", "testdata", "test3072.txt"), "rb") as f:
        s = fold_ref.mixed_case(f.read())
    orc = approx_ref.index_of(s)[0]
    rng = np.random.default_rng(302)
    general = fold_ref.make_map([b"abcdefgh", b"ij", b"xyz", b"TU"])
    for fold in (fold_ref.ASCII, general):
        table, cid = C.fold_table(fold)
        lib_cid, cls_off, mem_off, mem_bytes = unicode_fold.fold_map_table(fold)
        assert C.table_of(cls_off, mem_off, mem_bytes) == table and [c if c >= 0 else None for c in lib_cid] == cid
        for m in (0, 1, 2, 5, 12, 24):
            for at in rng.integers(0, len(s) - m, 3).tolist():
                p = s[at:at + m].swapcase()
                hits, steps, _ = C.walk(orc, C.folded(p, cid), table)
                assert [h[1:] for h in hits] == fold_ref.dfs_hits(orc, p, fold), p
                assert all(h[0] == m for h in hits)


# ---------------------------------------------------------------- the header
def test_abi_and_struct_sizes():
    assert _lib.load().fmx_abi_version() == 5
    assert ctypes.sizeof(_lib.fmx_class_table) == 40 and _lib.fmx_class_table.flags.offset == 32
    assert (_lib.FMX_CLASS_MAX_MEMBER_LEN, _lib.FMX_CLASS_MAX_MEMBERS, _lib.FMX_CLASS_MAX_ELEMS, _lib.FMX_CLASS_MAX_CLASSES) == (4, 16, 255, 65280)


@pytest.mark.skipif(shutil.which("gcc") is None, reason="needs gcc")
def test_struct_layout_against_a_strict_c_compile(tmp_path):
    src = tmp_path / "sizes.c"
    src.write_text(
        "#include <stddef.h>\n#include <stdio.h>\n#include <fmx.h>\n"
        "int main(void) {\n"
        "  printf(\"%d %d %d %d %d %d %d %d %d\\n\", (int)sizeof(fmx_class_table), (int)offsetof(fmx_class_table, n_classes),\n"
        "         (int)offsetof(fmx_class_table, flags), (int)offsetof(fmx_class_table, reserved), FMX_CLASS_MAX_MEMBER_LEN,\n"
        "         FMX_CLASS_MAX_MEMBERS, FMX_CLASS_MAX_ELEMS, FMX_CLASS_MAX_CLASSES, FMX_ABI_VERSION);\n"
        "  return 0;\n}\n")
    exe = tmp_path / "sizes"
    subprocess.check_call(["gcc", "-std=c99", "-Wall", "-Wextra", "-Werror", "-pedantic", "-I" + os.path.join(ROOT, "include"),
                           str(src), "-o", str(exe)])
    out = subprocess.run([str(exe)], capture_output=True, text=True, timeout=60)
    assert out.stdout.split() == ["40", "24", "32", "36", "4", "16", "255", "65280", "5"]


# ---------------------------------------------------------------- refusals that need no device
def table_struct(table, flags=0, reserved=0, n_classes=None):
    arrays = C.abi(table)
    t = _lib.fmx_class_table()
    t.cls_off, t.mem_off, t.mem_bytes = (a.ctypes.data for a in arrays)
    t.n_classes = len(table) if n_classes is None else n_classes
    t.flags, t.reserved = flags, reserved
    t._keep = arrays
    return t


BAD_TABLES = [
    ([[b"a", b"b"], [bytes([65 + j]) for j in range(17)]], b"class 1 has more than 16 members"),
    ([[b"a", b"abcde"]], b"class 0 has a member of more than 4 bytes"),
    ([[b"x"], [b"y"], [b"ab", b"abc"]], b"class 2 has a member that is a prefix of another"),
    ([[b"abc", b"ab"]], b"class 0 has a member that is a prefix of another"),
    ([[b"ab", b"c", b"ab"]], b"class 0 has the same member twice"),
    ([[b"a", b"b\0"]], b"class 0 has a member with byte 0"),
    ([[b"a"], []], b"class 1 has no member"),
    ([[b"a", b""]], b"class 0 has an empty member"),
]


def test_argument_refusals_before_any_device():
    """Everything the calls decide from their arguments alone comes before the handle is looked at, and the null handle is
    refused last with a message of its own: on a machine without a GPU each refusal still shows by its message."""
    L = _lib.load()
    n_out = ctypes.c_size_t(77)
    el = np.array([97, 256, 98, 257], dtype=np.uint16)
    off = np.array([0, 2, 4], dtype=np.uint64)
    out_off = np.zeros(3, dtype=np.uint64)
    out = np.zeros(4, dtype=[("regex", np.uint32), ("len", np.uint32), ("sp", np.uint64), ("ep", np.uint64)])
    good = table_struct([[b"a", b"bc"], [b"x", b"yz"]])

    def host(h=None, e=el, o=off, k=2, tab=good, cap=4, n=n_out, oo=out_off):
        return L.fmx_search_classes_batch(h, e.ctypes.data, o.ctypes.data, k, ctypes.byref(tab) if tab is not None else None,
                                          oo.ctypes.data if oo is not None else None, out.ctypes.data, cap,
                                          ctypes.byref(n) if n is not None else None)

    def dev(h=None, k=2, tab=good, cap=4, n=n_out):
        return L.fmx_search_classes_batch_dev(h, el.ctypes.data, off.ctypes.data, k, ctypes.byref(tab) if tab is not None else None,
                                              out_off.ctypes.data, out.ctypes.data, cap, ctypes.byref(n) if n is not None else None, None)

    cases = [(dict(), b"handle"), (dict(n=None), b"n_out"), (dict(tab=table_struct([[b"a"]], flags=1)), b"must be 0"),
             (dict(tab=table_struct([[b"a"]], reserved=9)), b"must be 0"), (dict(tab=table_struct([[b"a"]], n_classes=65281)), b"65280"),
             (dict(k=(1 << 26) + 1), b"2^26"), (dict(cap=1 << 32), b"2^32")]
    cases += [(dict(tab=table_struct(t)), word) for t, word in BAD_TABLES]
    for form in (host, dev):
        for kw, word in cases:
            assert form(**kw) == ARG, (form.__name__, kw)
            assert word in L.fmx_last_error(), (form.__name__, word, L.fmx_last_error())
        # the order: n_out, the table, k, cap, the null arguments, the handle
        assert form(n=None, tab=table_struct(BAD_TABLES[0][0]), k=1 << 27, cap=1 << 32) == ARG and b"n_out" in L.fmx_last_error()
        assert form(tab=table_struct(BAD_TABLES[0][0]), k=1 << 27, cap=1 << 32) == ARG and b"class 1" in L.fmx_last_error()
        assert form(k=1 << 27, cap=1 << 32) == ARG and b"2^26" in L.fmx_last_error()
        assert form(cap=1 << 32) == ARG and b"2^32" in L.fmx_last_error()
    assert host(o=np.array([0, 3, 2], dtype=np.uint64)) == ARG and b"non-decreasing" in L.fmx_last_error()
    assert host(oo=None) == ARG and b"null argument" in L.fmx_last_error()
    assert host(tab=None) == ARG and b"names class 0, the table has 0" in L.fmx_last_error()       # NULL: the empty table
    assert host(e=np.array([97, 258, 98, 257], dtype=np.uint16)) == ARG and b"names class 2" in L.fmx_last_error()
    assert host(e=np.array([97, 0, 98, 255], dtype=np.uint16), tab=None) == ARG and b"handle" in L.fmx_last_error()
    long_el = np.full(300, 97, dtype=np.uint16)
    assert host(e=long_el, o=np.array([0, 255, 256], dtype=np.uint64)) == ARG and b"handle" in L.fmx_last_error()      # 255 elements pass
    assert host(e=long_el, o=np.array([0, 256, 300], dtype=np.uint64)) == ARG and b"255 elements" in L.fmx_last_error()
    assert host(e=long_el, o=np.array([0, 256, 300], dtype=np.uint64), n=None) == ARG and b"255 elements" in L.fmx_last_error()      # the host form's first
    assert n_out.value == 77                                 # a refused call writes nothing
    a, b = ctypes.c_double(-1), ctypes.c_double(-1)
    c, d = ctypes.c_uint64(5), ctypes.c_uint64(5)
    assert L.fmx_classes_last(ctypes.byref(a), ctypes.byref(b), ctypes.byref(c), ctypes.byref(d)) == 0
    assert a.value >= 0 and b.value >= 0
    assert L.fmx_classes_last(None, None, None, None) == 0


# ---------------------------------------------------------------- the Unicode classes
def test_case_classes_against_re_ignorecase():
    classes = unicode_fold.case_classes()
    distinct = set(classes.values())
    assert 1300 < len(distinct) < 1500 and max(len(c) for c in distinct) == 4
    mixed = [c for c in distinct if len({len(chr(m).encode()) for m in c}) > 1]
    assert 30 <= len(mixed) <= 40
    for want in ((0x49, 0x69, 0x131), (0x4B, 0x6B, 0x212A), (0x53, 0x73, 0x17F), (0xC5, 0xE5, 0x212B), (0x3A3, 0x3C2, 0x3C3)):
        assert classes[want[0]] == want
    # inside a class every pair matches under re.IGNORECASE
    for c in distinct:
        for a in c:
            for b in c:
                assert re.fullmatch(re.escape(chr(a)), chr(b), re.IGNORECASE), (hex(a), hex(b))
    # and re.IGNORECASE equates nothing across classes: a code point matches the members of its own class only
    members = sorted(m for c in distinct for m in c)
    alphabet = "".join(chr(m) for m in members)
    for c in distinct:
        got = {ord(x) for x in re.findall(re.escape(chr(c[0])), alphabet, re.IGNORECASE)}
        assert got == set(c), [hex(m) for m in c]
    # a code point without a class matches itself alone
    for cp in (0x30, 0x5F, 0x149, 0x2116, 0x4E2D):
        assert cp not in classes and {ord(x) for x in re.findall(re.escape(chr(cp)), alphabet + chr(cp), re.IGNORECASE)} == {cp}
    assert unicode_fold.case_classes() is classes                                      # kept
    marks = unicode_fold.mark_classes()
    assert {ord(x) for x in "eEéÉêè"} <= set(marks[ord("e")]) and len(marks[ord("e")]) > 16


def test_tokeniser_and_class_table():
    T = unicode_fold.tokens
    assert T(b"a\xc3\xbc") == [(0x61, b"a"), (0xFC, b"\xc3\xbc")]
    assert T(b"\xff\xc3") == [(None, b"\xff"), (None, b"\xc3")]                        # a lead byte without its continuation
    assert T(b"\xc0\x80") == [(None, b"\xc0"), (None, b"\x80")]                        # overlong
    assert T(b"\xed\xa0\x80") == [(None, b"\xed"), (None, b"\xa0"), (None, b"\x80")]    # a surrogate
    assert T(b"\xe2\x84\xaak\xe2\x84") == [(0x212A, b"\xe2\x84\xaa"), (0x6B, b"k"), (None, b"\xe2"), (None, b"\x84")]
    assert T(b"\xf0\x9f\x98\x80") == [(0x1F600, b"\xf0\x9f\x98\x80")] and T(b"") == []
    el, off, cls_off, mem_off, mem_bytes = unicode_fold.class_table([b"k\xff1", b"", "Kü".encode()])
    table = C.table_of(cls_off, mem_off, mem_bytes)
    assert table == [[b"K", b"k", b"\xaa\x84\xe2"], [b"\x9c\xc3", b"\xbc\xc3"]]         # members reversed, by code point
    assert C.unpack(el, off) == [[0x31, 0xFF, 256], [], [257, 256]]                    # elements reversed; the same class once
    # pruning: one member left is inlined (reversed bytes), none left keeps the query's own bytes
    el, off, cls_off, mem_off, mem_bytes = unicode_fold.class_table([b"ks"], occurring={b"\xe2\x84\xaa"})
    assert C.unpack(el, off) == [[0x73, 0xAA, 0x84, 0xE2]] and cls_off.tolist() == [0] and mem_off.tolist() == [0]
    with pytest.raises(ValueError) as ei:
        unicode_fold.class_table([b"e"], unicode_fold.mark_classes())
    assert "'e'" in str(ei.value)
    el, off, cls_off, _, _ = unicode_fold.class_table([b"e"], unicode_fold.mark_classes(), occurring={b"e", b"\xc3\xa9", b"E"})
    assert C.unpack(el, off) == [[256]] and cls_off.tolist() == [0, 3]
    assert unicode_fold.members_of([b"k1"], unicode_fold.case_classes()) == [b"K", b"k", b"\xe2\x84\xaa"]


# ---------------------------------------------------------------- the command line
def test_rank_cli_parses_unicode_case():
    from findex_amd import rank as cli
    a = cli.parser().parse_args(["base", "q", "--unicode-case", "--ignore-marks"])
    assert a.unicode_case and a.ignore_marks and cli.flags_of(a) == {"ignore_case": "unicode", "ignore_marks": True}
    assert cli.flags_of(cli.parser().parse_args(["base", "q", "--unicode-case", "-i"])) == {"ignore_case": "unicode"}
    assert cli.flags_of(cli.parser().parse_args(["base", "q", "-i", "-w"])) == {"words": True, "ignore_case": True}      # -i stays ASCII
    assert cli.flags_of(cli.parser().parse_args(["base", "q"])) == {}
    assert cli.split_queries(["über K"], utf8=True) == [["über".encode("utf-8"), b"K"]]
    assert "--unicode-case" in cli.parser().format_help()
    assert cli.flags_of(cli.parser().parse_args(["base", "q", "--unicode-case", "-w"])) == {"words": True, "ignore_case": "unicode"}
    with pytest.raises(SystemExit):
        cli.main(["base", "q", "--ignore-marks"])


def test_grep_cli_parses_unicode_case():
    from findex_amd import grep as cli
    a = cli.parser().parse_args(["base", "re", "--unicode-case", "-w", "-n"])
    assert a.unicode_case and cli.flags_of(a) == {"words": True, "ignore_case": "unicode"} and cli.by_lines(a)
    assert cli.flags_of(cli.parser().parse_args(["base", "re", "--unicode-case", "-i"])) == {"ignore_case": "unicode"}
    assert cli.flags_of(cli.parser().parse_args(["base", "re", "-i"])) == {"ignore_case": True}          # -i stays ASCII
    assert cli.flags_of(cli.parser().parse_args(["base", "re", "--unicode-case", "--and", "x", "--not", "y"])) == {"ignore_case": "unicode"}
    assert cli.flags_of(cli.parser().parse_args(["base", "re"])) == {} and "--unicode-case" in cli.parser().format_help()


# ---------------------------------------------------------------- fold_regex_unicode
REGEX_TEXT = ("The Kelvin kelvin Kelvin KELVIN. über Über ÜBER üüber uber; miss miſs MISS mis ſtop stop STOP "
              "σοφίας ΣΟΦΊΑΣ σσ café CAFÉ cafe and AND anD an "
              "ıi I Å Å å the THE she SHE tHe")
REGEXES_U = ["über", "ÜBER", "k", "kelvin", "mis+", "σοφίασ", "(the|σ+)", "caf(é|e)", "[a-k]elvin",
             "ü+ber", "s?top", "an(d|D)?", "ı", "i", "å", "[s-u]h?e", "\\.", "(k|ü)(e|b)", "mi(s|ſ)*", "e(l|r)\\ "]
REFUSED_U = ["^the", "the$", "a{2}", "[^a]", "\\bthe", "\\n", "[\\d]", "[]", "[ü]", "[a-é]"]


def test_fold_regex_unicode_rewrites_and_refuses():
    from findex_amd.regex import fold_regex_unicode as f
    assert f("k") == "(K|k|\\â\\\u0084\\ª)" and f("ab") == "(A|a)(B|b)" and f("1.") == "(1)."
    assert f("ü+") == "(\\Ã\\\u009c|\\Ã\\¼)+"                      # the quantifier binds the character
    assert f("中*") == "(\\ä\\¸\\­)*"                               # ... also one without a class
    assert f("[a-c]") == "(A|B|C|a|b|c)" and "\\â\\\u0084\\ª" in f("[j-l]") and f("\\d") == "\\d" and f("\\w").startswith("(\\w|z|")
    assert f("cafe", ignore_marks=True) != f("cafe") and "\\Ã\\©" in f("cafe", ignore_marks=True)
    for rx in REGEXES_U:
        out = f(rx)
        assert out == f(rx) and all(ord(c) < 256 for c in out) and "[" not in out
    for rx in REFUSED_U:
        with pytest.raises(ValueError):
            f(rx)
    with pytest.raises(ValueError):
        f(b"abc")
    for rx in ("[a", "[a-", "[c-a]"):                        # re2post's own syntax errors are left for the compiler
        with pytest.raises(R.Re2PostSyntax):
            R.re2post(f(rx))


def test_fold_regex_unicode_against_python_re():
    """The oracle's NFA engine over reverse(REGEX_TEXT as UTF-8), given the rewritten regex, finds the strings re finds in the
    str under re.IGNORECASE.  First the alphabet: on the characters of the text re.IGNORECASE equates exactly the members of
    case_classes() -- no character such as U+0130, which re folds and the classes do not, is among them."""
    from findex_amd.regex import fold_regex_unicode
    classes = unicode_fold.case_classes()
    chars = sorted(set(REGEX_TEXT))
    for c in chars:
        got = {x for x in chars if re.fullmatch(re.escape(c), x, re.IGNORECASE)}
        assert got == {x for x in chars if ord(x) in classes.get(ord(c), (ord(c),))}, c
    data = REGEX_TEXT.encode("utf-8")
    orc = approx_ref.index_of(data[::-1])[0]

    class Index:
        n, getPrevRange = orc.n, orc.getPrevRange

    max_len = 12
    more = 0
    for rx in REGEXES_U:
        pat = re.compile(rx, re.IGNORECASE | re.DOTALL)
        want = set()
        s = REGEX_TEXT
        for a in range(len(s)):
            for b in range(a + 1, min(len(s), a + max_len) + 1):
                x = s[a:b].encode("utf-8")
                if len(x) <= max_len and pat.fullmatch(s, a, b):
                    r = orc.search(x[::-1])
                    assert r is not None
                    want.add((len(x), int(r[0]), int(r[1])))
        got = {(ln, sp, ep) for ln, sp, ep in E.nfa_matchSA(E.createNFA(R.re2post(fold_regex_unicode(rx))), Index, maxLength=max_len)}
        assert got == want, rx
        exact = {m for a in range(len(s)) for b in range(a + 1, min(len(s), a + max_len) + 1) for m in [s[a:b]] if re.fullmatch(rx, m, re.DOTALL)}
        more += len(want) > len({x for x in exact if len(x.encode()) <= max_len})
    assert more >= 12
