"""The corpus index without a GPU: the file order and the binary filter against DirBWTReader's rules, escaping, the checker the
GPU tests rest on (tests/corpus_ref.py) on the reference's own directories, the X.docs side file, the tool's --dir form, the
new symbols and their argument errors before any device is touched; the listing's reference helpers by hand, and the shapes
of the generated corpora of tests/corpus_many.py that tests/test_gpu_corpus_many.py relies on."""
import ctypes
import os
import re
import shutil
import subprocess
import sys

import numpy as np
import pytest

import corpus_many
import corpus_ref
import findex_amd
from conftest import ROOT, TESTDATA
from findex_amd import _lib, corpus, index


def _tree(tmp_path):
    """b.txt, a.txt, sub/z.txt, sub/deep/k.txt, Sub/m.txt, an empty file, a binary file, a file whose 0 sits at byte 1024."""
    (tmp_path / "sub" / "deep").mkdir(parents=True)
    (tmp_path / "Sub").mkdir()
    (tmp_path / "b.txt").write_bytes(b"bbb")
    (tmp_path / "a.txt").write_bytes(b"aaa")
    (tmp_path / "zz").write_bytes(b"last of the root's files")
    (tmp_path / "sub" / "z.txt").write_bytes(b"z")
    (tmp_path / "sub" / "deep" / "k.txt").write_bytes(b"k")
    (tmp_path / "Sub" / "m.txt").write_bytes(b"m")
    (tmp_path / "empty").write_bytes(b"")
    (tmp_path / "bin").write_bytes(b"x" * 1023 + b"\0")
    (tmp_path / "late0").write_bytes(b"x" * 1024 + b"\0")
    return tmp_path


def test_order_is_files_first_names_as_bytes(tmp_path):
    assert corpus.list_files(os.path.join(TESTDATA, "t1")) == [b"test1024-2.txt", b"test1024-3.txt", b"test1024.txt"]
    root = _tree(tmp_path)
    want = [b"a.txt", b"b.txt", b"late0", b"zz", b"Sub/m.txt", b"sub/z.txt", b"sub/deep/k.txt"]
    assert corpus.list_files(root) == want
    assert corpus_ref.walk(root) == want
    everything = [b"a.txt", b"b.txt", b"bin", b"empty", b"late0", b"zz", b"Sub/m.txt", b"sub/z.txt", b"sub/deep/k.txt"]
    assert corpus.list_files(root, filter_binary=False) == everything
    assert corpus_ref.walk(root, filter_binary=False) == everything


def test_is_binary_and_the_filter(tmp_path):
    root = _tree(tmp_path)
    assert corpus.is_binary(root / "bin")                     # a 0 within the first 1024 bytes
    assert not corpus.is_binary(root / "late0")               # a 0 at byte 1024 is not looked at
    assert corpus.is_binary(root / "empty")                   # an empty read is None: treated as binary
    assert corpus.is_binary(root / "no-such-file")            # cannot be opened
    assert not corpus.is_binary(root / "a.txt")
    for p in ("bin", "late0", "empty", "no-such-file", "a.txt"):
        assert corpus.is_binary(root / p) == corpus_ref.looks_binary(root / p)
    assert b"empty" not in corpus.list_files(root) and b"empty" in corpus.list_files(root, filter_binary=False)


def test_escape():
    assert corpus.escape(b"") == b""
    assert corpus.escape(b"a\x00b\x01c\xffd\\e") == b"a\\0b\\1c\\fd\\e"            # the backslash itself stays
    assert corpus.escape(bytes(range(256))) == corpus_ref.escape_bytes(bytes(range(256)))
    assert len(corpus.escape(bytes(range(256)))) == 259
    L = _lib.load()
    src = np.frombuffer(b"\xff\xff", dtype=np.uint8)
    out = np.full(8, 7, dtype=np.uint8)
    n = ctypes.c_size_t()
    assert L.fmx_corpus_escape(src.ctypes.data, 2, out.ctypes.data, 3, ctypes.byref(n)) == 9 and n.value == 4       # FMX_ERR_OVERFLOW
    assert np.all(out == 7)
    assert L.fmx_corpus_escape(src.ctypes.data, 2, out.ctypes.data, 4, ctypes.byref(n)) == 0 and bytes(out[:4]) == b"\\f\\f"


def test_reference_streams():
    t1 = corpus_ref.RefCorpus.from_dir(os.path.join(TESTDATA, "t1"))
    assert len(t1.stream) == 3075 and t1.stream[0] == 67 and t1.stream[1] == 67            # "CC": test1024-2.txt comes first
    assert t1.doc_start == [0, 1025, 2050, 3075] and t1.esc_pos == []
    assert [t1.stream[p] for p in (1024, 2049, 3074)] == [1, 1, 1]
    tbad = corpus_ref.RefCorpus.from_dir(os.path.join(TESTDATA, "tbad"))
    assert [d.count(b"\xff") for d in tbad.docs] == [48, 39, 46]
    assert len(tbad.stream) == 3 * 1024 + 133 + 3 and len(tbad.esc_pos) == 133
    assert tbad.stream.count(b"\x01") == 3 and b"\xff" not in tbad.stream and b"\0" not in tbad.stream
    # the per-position table: both bytes of an escape stand for one raw byte, a separator for the raw length
    e = tbad.esc_pos[0]
    assert tbad.stream[e:e + 2] == b"\\f" and tbad.table[e][2] == tbad.table[e + 1][2] and tbad.docs[0][tbad.table[e][2]] == 255
    assert tbad.table[tbad.doc_start[1] - 1] == (0, 1024 + 48, 1024)
    assert tbad.map(len(tbad.stream)) == (0xFFFFFFFF, 2 ** 64 - 1, 2 ** 64 - 1)
    c = corpus_ref.RefCorpus([b"", b"a\x00", b""])
    assert c.stream == b"\x01a\\0\x01\x01" and c.doc_start == [0, 1, 5, 6] and c.esc_pos == [2] and c.raw_len == [0, 2, 0]
    assert c.table == [(0, 0, 0), (1, 0, 0), (1, 1, 1), (1, 2, 1), (1, 3, 2), (2, 0, 0)]


def test_docs_file_round_trip_and_refusals(tmp_path):
    ref = corpus_ref.RefCorpus.from_dir(os.path.join(TESTDATA, "tbad"))
    p = tmp_path / "x.docs"
    corpus.write_docs(p, ref.doc_start, ref.raw_len, ref.esc_pos, ref.names)
    blob = p.read_bytes()
    assert blob[:8] == b"FMXDOCS1" and len(blob) == 32 + 8 * (4 + 3 + 133 + 4) + sum(len(n) for n in ref.names)
    assert np.frombuffer(blob, dtype="<u8", count=3, offset=8).tolist() == [3, 133, len(ref.stream)]
    ds, rl, ep, names = corpus.read_docs(p)
    assert ds.tolist() == ref.doc_start and rl.tolist() == ref.raw_len and ep.tolist() == ref.esc_pos and names == ref.names
    for cut in (0, 7, 31, 40, len(blob) - 1):
        (tmp_path / "cut.docs").write_bytes(blob[:cut])
        with pytest.raises(ValueError):
            corpus.read_docs(tmp_path / "cut.docs")
        with pytest.raises(ValueError):                       # Corpus.load refuses it before it asks for a device
            corpus.Corpus.load(tmp_path / "cut.docs")
    (tmp_path / "magic.docs").write_bytes(b"FMXDOCS2" + blob[8:])
    with pytest.raises(ValueError):
        corpus.Corpus.load(tmp_path / "magic.docs")
    (tmp_path / "long.docs").write_bytes(blob + b"x")
    with pytest.raises(ValueError):
        corpus.read_docs(tmp_path / "long.docs")


def _cli(*args):
    env = dict(os.environ)
    env["PYTHONPATH"] = ROOT + os.pathsep + env.get("PYTHONPATH", "")
    return subprocess.run([sys.executable, "-m", "findex_amd.index"] + list(args), cwd=ROOT, env=env, capture_output=True,
                          text=True, timeout=300)


def test_tool_dir_form(tmp_path):
    r = _cli("--dir", os.path.join(TESTDATA, "t1"))
    assert r.returncode == 2 and "--out" in r.stderr
    r = _cli("--dir", os.path.join(TESTDATA, "t1"), "--out", str(tmp_path / "x"), "extra.txt")
    assert r.returncode == 2
    r = _cli("--out", str(tmp_path / "x"))
    assert r.returncode == 2
    assert not list(tmp_path.iterdir())
    a = index.parser().parse_args(["--dir", "D", "--out", "o/X"])
    assert index.planned_outputs(a) == ["o/X.bwt", "o/X.aux", "o/X.docs"]
    a = index.parser().parse_args(["--dir", "D", "--out", "o/X.v1", "--data", "--no-filter-binary", "--fm", "--sa", "--lcp"])
    assert index.planned_outputs(a) == ["o/X.v1.bwt", "o/X.v1.aux", "o/X.v1.docs", "o/X.v1.data", "o/X.v1.fm", "o/X.v1.sa", "o/X.v1.lcp"]
    assert a.no_filter_binary and a.data
    # the single-file form is what it was
    a = index.parser().parse_args(["dir/X.txt", "--lcp"])
    assert a.dir is None and index.planned_outputs(a) == ["dir/X.bwt", "dir/X.aux", "dir/X.lcp"]


def _declared():
    text = open(os.path.join(ROOT, "include", "fmx.h")).read()
    text = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    return sorted(set(re.findall(r"\b(fmx_corpus_[a-z0-9_]+)\s*\(", text)))


def test_new_symbols_are_declared_bound_and_exported():
    names = _declared()
    assert {"fmx_corpus_build", "fmx_corpus_build_dev", "fmx_corpus_info", "fmx_corpus_stream", "fmx_corpus_stream_dev",
            "fmx_corpus_drop_stream", "fmx_corpus_open_index", "fmx_corpus_tables", "fmx_corpus_from_tables", "fmx_corpus_map",
            "fmx_corpus_map_dev", "fmx_corpus_doc_list", "fmx_corpus_doc_list_dev", "fmx_corpus_free",
            "fmx_corpus_escape"} <= set(names)
    L = ctypes.CDLL(_lib.LIB_PATH)
    for nm in names:
        assert nm in _lib.SYMBOLS and hasattr(L, nm), nm
    for nm in ("Corpus", "HipCorpusSearcher", "escape", "is_binary", "list_files"):
        assert nm in findex_amd.__all__ and hasattr(findex_amd, nm)


@pytest.mark.skipif(shutil.which("gcc") is None, reason="needs gcc")
def test_header_stays_c99_with_the_corpus_calls(tmp_path):
    src = tmp_path / "use_corpus.c"
    src.write_text(
        "#include <fmx.h>\n"
        "int main(void) {\n"
        "  fmx_corpus *c = 0; fmx_index *ix = 0; uint64_t ends[1] = {3}, n = 0; uint32_t tile = 0; size_t m = 0;\n"
        "  uint8_t out[8];\n"
        "  if (fmx_corpus_free(c) != FMX_OK) return 2;\n"
        "  if (fmx_corpus_info(c, &n, 0, 0, 0, 0, &tile) != FMX_OK || tile == 0) return 3;\n"
        "  if (fmx_corpus_escape((const uint8_t *)\"a\\1\", 2, out, 8, &m) != FMX_OK || m != 3) return 4;\n"
        "  if (fmx_corpus_build((const uint8_t *)\"abc\", 3, ends, 0, 0, &c) != FMX_ERR_ARG) return 5;\n"
        "  if (fmx_corpus_open_index(c, 0, &ix) != FMX_ERR_ARG) return 6;\n"
        "  return 0;\n}\n")
    inc = os.path.join(ROOT, "include")
    subprocess.check_call(["gcc", "-std=c99", "-Wall", "-Wextra", "-Werror", "-pedantic", "-I" + inc, "-c", str(src), "-o",
                           str(tmp_path / "a.o")])
    libdir = os.path.dirname(_lib.LIB_PATH)
    exe = tmp_path / "use_corpus"
    subprocess.check_call(["gcc", str(tmp_path / "a.o"), "-L" + libdir, "-lfmx", "-Wl,-rpath," + libdir, "-Wl,-rpath,/opt/rocm/lib",
                           "-o", str(exe)])
    r = subprocess.run([str(exe)], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, (r.returncode, r.stderr[-500:])


def test_argument_errors_before_any_device():
    L = _lib.load()
    h = ctypes.c_void_p()
    raw = np.frombuffer(b"abcdef", dtype=np.uint8)
    u64 = lambda *v: np.array(v, dtype=np.uint64)          # noqa: E731
    build = lambda ends, n_docs, raw_len=6: L.fmx_corpus_build(raw.ctypes.data, raw_len, ends.ctypes.data, n_docs, 0, ctypes.byref(h))      # noqa: E731
    assert build(u64(6), 0) == 3                                          # no document
    assert build(u64(4, 3, 6), 3) == 3 and b"decrease" in L.fmx_last_error()
    assert build(u64(2, 5), 2) == 3 and b"end" in L.fmx_last_error()      # the last end is not the raw length
    assert L.fmx_corpus_build(None, 6, u64(6).ctypes.data, 1, 0, ctypes.byref(h)) == 3
    assert L.fmx_corpus_build(raw.ctypes.data, 6, None, 1, 0, ctypes.byref(h)) == 3
    assert L.fmx_corpus_build(raw.ctypes.data, 6, u64(6).ctypes.data, 1, 0, None) == 3
    assert L.fmx_corpus_build(raw.ctypes.data, 1 << 32, u64(1 << 32).ctypes.data, 1, 0, ctypes.byref(h)) == 6      # FMX_ERR_UNSUPPORTED
    assert b"2^32 - 2" in L.fmx_last_error()
    assert L.fmx_corpus_free(None) == 0
    assert L.fmx_corpus_map(None, None, 0, None, None, None) == 3
    assert L.fmx_corpus_stream(None, None, 0) == 3 and L.fmx_corpus_drop_stream(None) == 3
    assert L.fmx_corpus_tables(None, None, None, None) == 3
    # tables that contradict each other: FMX_ERR_FORMAT, decided on the host
    ft = lambda ds, rl, ep: L.fmx_corpus_from_tables(ds.ctypes.data, rl.ctypes.data, ep.ctypes.data if ep.size else None, rl.size,      # noqa: E731
                                                     ep.size, 0, ctypes.byref(h))
    none = np.zeros(0, dtype=np.uint64)
    assert ft(u64(1, 4), u64(2), none) == 2                               # doc_start[0] != 0
    assert ft(u64(0, 3, 3), u64(2, 0), none) == 2                         # not strictly increasing
    assert ft(u64(0, 4), u64(2), none) == 2                               # raw_len disagrees: 3 bytes and a separator
    assert ft(u64(0, 4), u64(2), u64(2)) == 2                             # an escape whose second byte is the separator
    assert ft(u64(0, 6), u64(3), u64(1, 2)) == 2                          # escapes that overlap
    rc = ft(u64(0, 4), u64(2), u64(1))                                    # consistent: goes on to the device
    assert rc in (0, 5), L.fmx_last_error()
    if rc == 0:
        L.fmx_corpus_free(h)
    else:
        assert b"no CPU fallback" in L.fmx_last_error()
        with pytest.raises(findex_amd.FmxError):
            findex_amd.Corpus.from_documents([b"abc"])


# ---- the listing's reference helpers and the corpora of tests/test_gpu_corpus_many.py
def test_doc_counts_and_list_positions_by_hand():
    docs = [b"\x00aa\xff", b"", b"aaa", b"b\x01aab", b"\\a"]
    ref = corpus_ref.RefCorpus(docs)
    assert ref.stream == b"\\0aa\\f\x01" b"\x01" b"aaa\x01" b"b\\1aab\x01" b"\\a\x01"
    assert ref.doc_start == [0, 7, 8, 12, 19, 22] and ref.esc_pos == [0, 4, 13]
    # a query that overlaps itself: "aa" stands twice in "aaa"
    assert ref.occurrences(b"aa") == [(0, 1), (2, 0), (2, 1), (3, 2)]
    assert ref.doc_counts(b"aa") == [(0, 1), (2, 2), (3, 1)]
    assert ref.doc_counts(b"a") == [(0, 2), (2, 3), (3, 2), (4, 1)]
    assert ref.doc_counts(b"\x00") == [(0, 1)] and ref.doc_counts(b"\xff") == [(0, 1)] and ref.doc_counts(b"\x01a") == [(3, 1)]
    assert ref.doc_counts(b"\\") == [(4, 1)] and ref.doc_counts(b"zz") == [] and ref.doc_counts(b"ab") == [(3, 1)]
    # positions: both bytes of the escapes at a document's first and last byte, separators (the empty document's too), None
    assert ref.list_positions([]) == []
    assert ref.list_positions([0, 1, 4, 5, 6]) == [(0, 5)]
    assert ref.list_positions([7]) == [(1, 1)]
    assert ref.list_positions([21, 7, None, 8, 0, 10, None, 11, 19, 12]) == [(0, 1), (1, 1), (2, 3), (3, 1), (4, 2), (0xFFFFFFFF, 2)]
    assert ref.list_positions([None]) == [(0xFFFFFFFF, 1)]
    assert ref.list_positions(range(len(ref.stream))) == [(0, 7), (1, 1), (2, 4), (3, 7), (4, 3)]
    assert corpus_many.expected_doc_counts(ref, b"\\") == [(0, 2), (3, 1), (4, 1)]
    assert corpus_many.expected_occurrences(ref, b"\\") == [(0, 0), (0, 3), (3, 1), (4, 0)]
    off, doc, cnt = corpus_many.csr([[(0, 1), (2, 2)], [], [(4, 7)]])
    assert off.tolist() == [0, 2, 2, 3] and doc.tolist() == [0, 2, 4] and cnt.tolist() == [1, 2, 7]
    assert doc.dtype == np.uint32 and cnt.dtype == np.uint32 and off.dtype == np.uint64


def _stream_finds(ref, esc):
    out, i = [], ref.stream.find(esc)
    while i >= 0:
        out.append(i)
        i = ref.stream.find(esc, i + 1)
    return out


@pytest.fixture(scope="module")
def many():
    return {name: corpus_ref.RefCorpus(corpus_many.documents(name)) for name in corpus_many.CORPORA}


def test_doc_counts_equal_the_listing_of_the_stream_positions(many):
    """For a query without a backslash the escaped query stands in the stream exactly where the query stands in the files."""
    for name in ("D256", "D5000"):
        ref = many[name]
        for q in corpus_many.QUERIES:
            if b"\\" in q:
                continue
            assert ref.doc_counts(q) == ref.list_positions(_stream_finds(ref, corpus_ref.escape_bytes(q))), (name, q)
        # the lone backslash: every escape pair begins with one (the union corpus_many states)
        assert corpus_many.expected_doc_counts(ref, b"\\") == ref.list_positions(_stream_finds(ref, b"\\"))


def test_many_document_corpora_have_the_shapes_their_tests_are_for(many):
    bits = {"D255": 8, "D256": 9, "D257": 9, "D5000": 13, "D65537": 17}
    for name, ref in many.items():
        n_docs = corpus_many.CORPORA[name][0]
        assert len(ref.docs) == n_docs and corpus_many.lib_bits(n_docs) == bits[name]
        assert len(ref.stream) < 1 << 20
        for c in (b"0", b"1", b"f"):                              # no raw text reads like an escape pair
            assert all(c not in d for d in ref.docs)
        # the documents placed by hand
        for at, placed in corpus_many.hand_placed(n_docs).items():
            assert ref.docs[at:at + len(placed)] == placed
        a, b, c = n_docs // 3, n_docs // 2, (2 * n_docs) // 3
        assert ref.docs[0] == b"" and ref.docs[-1] == b"" and ref.docs[c:c + 3] == [b"", b"", b""]
        assert ref.docs[a] in (b"\x00", b"\x01", b"\xff") and len(ref.docs[a + 2]) == 1 and len(ref.docs[a + 3]) == 1
        assert ref.doc_start[a] in ref.esc_pos and ref.doc_start[a + 2] in ref.esc_pos and ref.doc_start[a + 3] in ref.esc_pos
        assert ref.doc_start[b] in ref.esc_pos and ref.doc_start[b + 3] - 3 in ref.esc_pos
        empty = sum(1 for d in ref.docs if not d)
        mean = sum(ref.raw_len) / n_docs
        if name == "D65537":
            assert 0.45 * n_docs < empty < 0.55 * n_docs and 1.5 < mean < 2.5
        else:
            assert 0.02 * n_docs < empty < 0.10 * n_docs and 22 < mean < 34
    # D5000 under the query set: a second radix tile, listings of hundreds of documents, empty documents between hits, misses
    ref = many["D5000"]
    per = {q: corpus_many.expected_doc_counts(ref, q) for q in corpus_many.QUERIES}
    assert max(sum(c for _, c in p) for p in per.values()) > 4096
    assert max(len(p) for p in per.values()) > 256
    assert sum(1 for p in per.values() if not p) >= 1 and all(per[q] == [] for q in corpus_many.MISSES)
    skips = 0
    for p in per.values():
        for (d0, _), (d1, _) in zip(p, p[1:]):
            skips += any(not ref.docs[d] for d in range(d0 + 1, d1))
    assert skips >= 1
    assert len(set(corpus_many.QUERIES)) == len(corpus_many.QUERIES) == 4 + 16 + 64 + 6 + 2
    # the escaped lengths that share a listing call: 1-grams with the backslash, ..., a miss among the 3-grams, a call of misses only
    by_len = {}
    for q in corpus_many.QUERIES:
        by_len.setdefault(len(corpus_ref.escape_bytes(q)), []).append(q)
    assert sorted(by_len) == [1, 2, 3, 4] and b"azb" in by_len[3] and by_len[4] == [b"abzd"]


def test_key_width_cases_reach_their_bits_and_rows(many):
    for name, k, bits, passes in corpus_many.WIDTH_CASES:
        ref = many[name]
        assert corpus_many.lib_bits(len(ref.docs)) + corpus_many.lib_bits(k) == bits and (bits + 7) // 8 == passes
        g, tokens, rows = corpus_many.width_case(ref, k)
        assert len(tokens) == k and rows <= corpus_many.MAX_ROWS
        counts = corpus_many.gram_counts(ref, g)
        assert rows == sum(counts[w] for kind, w in tokens if kind == "hit")
        for w in sorted({w for kind, w in tokens if kind == "hit"})[:8]:      # the sizing pass counts what the reference finds
            assert counts[w] == len(ref.occurrences(w)) > 0
        if k > 1:
            kinds = [kind for kind, _ in tokens]
            assert kinds[0] == "miss" and kinds[-1] == "miss" and "inverted" in kinds and "miss" in kinds[1:-1]
            hits = {w for kind, w in tokens if kind == "hit"}
            assert len(hits) >= 4
            # the top bit of the key is in use unless k is a power of two: the last interval with rows has it set
            last = max(i for i, (kind, _) in enumerate(tokens) if kind == "hit")
            assert (corpus_many.lib_bits(last) == corpus_many.lib_bits(k)) == (k & (k - 1) != 0)
        if name != "D255":
            assert rows > 4096 * 16                               # many radix tiles, a scan with block totals
        if name in ("D5000", "D65537"):
            assert rows >= 1 << 20
    assert {("D255", 1, 9, 2), ("D256", 127, 16, 2), ("D256", 128, 17, 3), ("D5000", 2047, 24, 3), ("D5000", 2048, 25, 4),
            ("D5000", 70000, 30, 4), ("D65537", 40000, 33, 5)} <= set(corpus_many.WIDTH_CASES)
