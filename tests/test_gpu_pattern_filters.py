"""K6 pattern leaves: contains, ends_with and LIKE / NOT LIKE with `%` on VARCHAR / BLOB columns, pushed into the scan
(kLeafStrMatch, the third instance of the filter kernel), with selection vectors and with late materialisation.  The
reference pushes no filters (filter_pushdown = false, src/scanner/read_arrow.cpp:47-48) and DuckDB's filter above the scan
keeps the same rows, so every case is checked against Python's own evaluation of pyarrow's values -- `needle in row`,
row.endswith(suffix), re.fullmatch of the pattern with each `%` -> `.*` under re.DOTALL, NULL -> false -- never against the
code under test.  The kernel scans a row by its own lane whatever its length: there is no wave path and no threshold to
place needles around."""
import re

import numpy as np
import pyarrow as pa
import pyarrow.ipc as ipc
import pytest

import duckdb_arrow_amd as da

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def con():
    return da.Connection(0)


def as_bytes(v):
    return v.encode() if isinstance(v, str) else bytes(v)


def like_regex(pattern):
    return re.compile(b"".join(b".*" if c == 0x25 else re.escape(bytes([c])) for c in as_bytes(pattern)), re.DOTALL)


def is_tree(e):
    return e[0] in ("and", "or") and len(e) > 1 and isinstance(e[1], tuple)


def python_says(expr, cols, i):
    """Python's own evaluation of the predicate on row i; a comparison with NULL is not true"""
    if is_tree(expr):
        rs = [python_says(e, cols, i) for e in expr[1:]]
        return all(rs) if expr[0] == "and" else any(rs)
    v, op = cols[expr[0]][i], expr[1]
    if op == "is null":
        return v is None
    if op == "is not null":
        return v is not None
    if v is None:
        return False
    if isinstance(v, (str, bytes)):
        v = as_bytes(v)
        if op == "in":
            return v in [as_bytes(c) for c in expr[2]]
        c = as_bytes(expr[2])
        if op == "contains":
            return c in v
        if op == "ends_with":
            return v.endswith(c)
        if op == "starts_with":
            return v.startswith(c)
        if op in ("like", "not like"):
            return (like_regex(c).fullmatch(v) is not None) == (op == "like")
    elif op == "in":
        return v in expr[2]
    else:
        c = expr[2]
    return {"=": v == c, "<>": v != c, "<": v < c, "<=": v <= c, ">": v > c, ">=": v >= c}[op]


def leaf_columns(expr):
    return {c for e in expr[1:] for c in leaf_columns(e)} if is_tree(expr) else {expr[0]}


def wanted(expr, table, degenerate=False):
    """The rows Python keeps.  Unless the case is one of the named degenerate ones, the predicate must keep at least one row
    and drop at least one row whose filter columns are not NULL: a case that keeps everything or nothing shows nothing."""
    cols = {name: table.column(name).to_pylist() for name in table.column_names}
    want = [i for i in range(table.num_rows) if python_says(expr, cols, i)]
    if not degenerate:
        kept = set(want)
        dropped = [i for i in range(table.num_rows) if i not in kept and all(cols[c][i] is not None for c in leaf_columns(expr))]
        assert want and dropped, ("degenerate case", expr, len(want), len(dropped))
    return cols, want


def write(path, table, **kw):
    options = kw.pop("options", None)
    with (ipc.new_stream(path, table.schema, options=options) if options else ipc.new_stream(path, table.schema)) as w:
        w.write_table(table, **kw)
    return path


def check(con, path, table, expr, project, degenerate=False, compact=(False, True), **kw):
    """the selected rows of `project` (its first column numbers the rows), with a selection vector and compacted"""
    cols, want = wanted(expr, table, degenerate)
    for c in compact:
        got = con.read_arrow(path, filter_compact=c, **kw).project(project).filter(expr).fetch_columns()
        assert got[0] == want, (expr, c, len(got[0]), len(want))
        for name, g in zip(project[1:], got[1:]):
            assert g == [cols[name][i] for i in want], (expr, c, name)
    return want


# ----------------------------------------------------------------------------------------------- the inline boundary
NEEDLE_LENGTHS = [1, 2, 3, 4, 5, 8, 12, 13]
NEEDLES = {n: bytes(range(0x61, 0x61 + n)) for n in NEEDLE_LENGTHS}     # abcdefghijklm: no %, no _


def boundary_rows():
    """Rows of every length 0 .. 20 around every needle: the hit starts at byte 0, ends at the last byte, straddles byte 4 (the
    end of string_t's prefix) and byte 12 (the end of an inline string), is absent by one byte, or is the whole row."""
    fill = lambda k: bytes(0x51 + (j % 3) for j in range(k))            # QRS...: shares no byte with a needle
    rows = [None, b""]
    for n, needle in NEEDLES.items():
        near = needle[:-1] + bytes([needle[-1] + 1])                       # absent by one byte
        rows += [needle, near, needle[:-1], needle[1:]]
        for length in range(n + 1, 21):
            free = length - n
            for at in {0, free, 3, 11, 4 - n + 1, 12 - n + 1, 4, 12}:
                if 0 <= at <= free:
                    rows.append(fill(at) + needle + fill(free - at))
                    rows.append(fill(at) + near + fill(free - at))
            rows.append(fill(length))
            if 2 * n + 2 <= length:
                rows += [fill(1) + needle + needle + fill(length - 2 * n - 1), needle + fill(length - 2 * n) + needle]
            rows.append(needle[: n // 2 + 1] + fill(free - 1) + needle[n // 2:] if n > 1 else fill(length))   # the needle torn apart
        rows.append(None)
    return rows


@pytest.fixture(scope="module")
def boundary(tmp_path_factory):
    rows = boundary_rows()
    lengths = {len(r) for r in rows if r is not None}
    assert lengths == set(range(21)) and rows.count(None) > 5 and len(rows) < 30000
    t = pa.table({"k": pa.array(np.arange(len(rows), dtype=np.int64)), "s": pa.array(rows, pa.binary())})
    return write(str(tmp_path_factory.mktemp("bnd") / "b.arrows"), t, max_chunksize=700), t


@pytest.mark.parametrize("n", NEEDLE_LENGTHS)
def test_inline_boundary(con, boundary, n):
    path, t = boundary
    needle = NEEDLES[n]
    rows = [r for r in t.column("s").to_pylist() if r is not None]
    # the placements the fixture promises for this needle are there
    assert any(r.startswith(needle) and len(r) > n for r in rows) and any(r.endswith(needle) and len(r) > n for r in rows)
    straddles = lambda b: any(0 <= r.find(needle) < b < r.find(needle) + n for r in rows)    # bytes b - 1 and b are both in the hit
    assert needle in rows and (n == 1 or (straddles(4) and straddles(12)))
    assert any(r[3:3 + n] == needle for r in rows) and (n > 9 or any(r[11:11 + n] == needle for r in rows))
    for expr in [("s", "contains", needle), ("s", "ends_with", needle), ("s", "like", b"%" + needle + b"%"), ("s", "like", b"%" + needle),
                 ("s", "not like", b"%" + needle + b"%"), ("s", "like", b"Q%" + needle + b"%Q"), ("s", "like", b"%" + needle + b"%" + needle + b"%")]:
        degenerate = expr[2].count(needle) == 2 and 2 * n + 2 > 20    # longer than every row: keeps nothing
        check(con, path, t, expr, ["k", "s"], degenerate=degenerate)


def test_degenerate_needles(con, boundary):
    """the named degenerate cases: the empty needle and '%' keep every row that is not NULL, a needle longer than every row none"""
    path, t = boundary
    not_null = t.num_rows - t.column("s").null_count
    for expr, n_want in [(("s", "contains", b""), not_null), (("s", "ends_with", b""), not_null), (("s", "like", b"%"), not_null),
                         (("s", "like", b"%%%"), not_null), (("s", "not like", b"%"), 0), (("s", "contains", b"a" * 21), 0),
                         (("s", "ends_with", b"Q" * 21), 0), (("s", "like", b"%" + b"Q" * 21 + b"%"), 0)]:
        want = check(con, path, t, expr, ["k", "s"], degenerate=True)
        assert len(want) == n_want, expr


# ----------------------------------------------------------------------------------------------- order, overlap, backtracking
ORDER_ROWS = ["aaab", "aab", "aaa", "abababa", "ababab", "abab", "aba", "a", "aa", "abc", "abbc", "abcabc", "abcab", "ababa", "ab", "b", "",
              None, "xaaabx", "bbbbbbbbbbbbbbaaab", "aaaaaaaaaaaaaaaaaaaab", "aaaaaaaaaaaaaaaaaaaa", "abababababababababa", "abcabcabcabcabcab",
              "ab" * 9 + "bc", "a" * 13, "a" + "b" * 14 + "a", "x" * 13 + "abab", "x" * 13 + "aba", None]
ORDER_CASES = [("contains", "aab"), ("contains", "abab"), ("like", "%ab%ab%"), ("like", "a%a"), ("like", "ab%bc"), ("like", "%abc"),
               ("like", "%aba%ba%"), ("like", "%%a%%b%%"), ("like", "%a%b%"), ("not like", "%ab%ab%"), ("not like", "a%a"),
               ("ends_with", "aab"), ("like", "%aab"), ("like", "a%b%a%b%a"), ("like", "%a%a%a%a%a%a%a%a%")]


@pytest.fixture(scope="module")
def order_table(tmp_path_factory):
    t = pa.table({"k": pa.array(np.arange(len(ORDER_ROWS), dtype=np.int64)), "s": pa.array(ORDER_ROWS, pa.string())})
    return write(str(tmp_path_factory.mktemp("ord") / "o.arrows"), t), t


@pytest.mark.parametrize("op,pattern", ORDER_CASES, ids=["%s %s" % c for c in ORDER_CASES])
def test_backtracking_segment_order_and_overlap(con, order_table, op, pattern):
    path, t = order_table
    want = check(con, path, t, ("s", op, pattern), ["k", "s"])
    kept = {ORDER_ROWS[i] for i in want}
    # what the issue spells out, through Python's answer: the named rows are in or out
    named = {("contains", "aab"): (["aaab"], []), ("contains", "abab"): (["abababa"], ["aba"]), ("like", "%ab%ab%"): (["abab"], ["aba"]),
             ("like", "a%a"): (["aa"], ["a"]), ("like", "ab%bc"): (["abbc"], ["abc"]), ("like", "%abc"): (["abcabc"], ["abcab"]),
             ("like", "%aba%ba%"): (["ababa"], ["abab"])}.get((op, pattern), ([], []))
    assert all(r in kept for r in named[0]) and not any(r in kept for r in named[1])
    if pattern == "%%a%%b%%":
        assert want == wanted(("s", "like", "%a%b%"), t)[1]


# ----------------------------------------------------------------------------------------------- neighbours in the heap
@pytest.mark.parametrize("last_row_ends_the_buffer", [False, True])
def test_a_match_never_reaches_into_the_next_row(con, tmp_path, last_row_ends_the_buffer):
    """Consecutive long rows in one pyarrow-written buffer: row i ends with ...spe and row i + 1 begins with cial...; neither
    contains `special`, neither ends with it, and %spe%cial% matches neither."""
    rows = []
    for i in range(600):
        pad = "p" * (13 + i % 9)          # every alignment of the seam
        rows += [pad + "spe", "cial" + pad, pad + " special " + pad, pad + "special", "spe" + pad + "cial" + pad, pad + "cial spe"]
    rows += ["the last row is long and ends in spe"] if last_row_ends_the_buffer else ["cial to close the column"]
    arr = pa.array(rows, pa.string())
    data = arr.buffers()[2]
    assert data.size == sum(len(r) for r in rows)            # one buffer, the rows back to back, the last one at its end
    assert data.to_pybytes().startswith((rows[0] + rows[1]).encode()) and "special" in rows[0] + rows[1]   # the seam spells the needle
    t = pa.table({"k": pa.array(np.arange(len(rows), dtype=np.int64)), "s": arr})
    path = write(str(tmp_path / "n.arrows"), t)
    for expr in [("s", "contains", "special"), ("s", "ends_with", "special"), ("s", "like", "%spe%cial%"), ("s", "not like", "%spe%cial%"),
                 ("s", "ends_with", "spe"), ("s", "like", "%pspe%"), ("s", "contains", "spec")]:
        want = check(con, path, t, expr, ["k", "s"])
        if expr[1] != "not like" and expr[2] in ("special", "%spe%cial%"):
            assert not any(rows[i].endswith("pspe") or rows[i].startswith("cialp") or rows[i].startswith("cial to") for i in want)


# ----------------------------------------------------------------------------------------------- row-count seams
@pytest.mark.parametrize("n", [1, 2047, 2048, 2049, 8192, 8193])
def test_row_count_seams(con, tmp_path, n):
    """a window is 2048 rows, a workgroup takes 4 of them"""
    words = ["regular", "special deposits", "the special requests", "", None, "quickly final packages", "requests special",
             "s", "x" * 30 + "special", "special" + "y" * 30]
    rows = [words[(i * 7 + i // 11) % len(words)] for i in range(n)]
    rows[0] = "not that one"
    rows[-1] = "the very last row is special"                # n == 1: the only row, kept by two of the three predicates
    t = pa.table({"k": pa.array(np.arange(n, dtype=np.int64)), "s": pa.array(rows, pa.string())})
    path = write(str(tmp_path / "r.arrows"), t)               # one record batch
    for expr in [("s", "contains", "special"), ("s", "like", "%special%requests%"), ("s", "ends_with", "special")]:
        want = check(con, path, t, expr, ["k", "s"], degenerate=n == 1)
        if expr[1] != "like":
            assert want[-1] == n - 1


# ----------------------------------------------------------------------------------------------- long rows
@pytest.mark.parametrize("size", [70000, 1 << 20])
def test_long_rows(con, tmp_path, size):
    """Three-row files: the needle at the very start, at the very end, absent.  A row is scanned by its own lane whatever its
    length, so there is no round boundary to walk the needle across."""
    needle = b"NEEDLE-0123456789"
    body = bytes(0x61 + (j * 7 + j // 13) % 23 for j in range(size))          # no N, no digits
    rows = [needle + body[len(needle):], body[:-len(needle)] + needle, body[:-1] + b"N"]
    assert [len(r) for r in rows] == [size] * 3 and needle not in rows[2]
    t = pa.table({"k": pa.array(np.arange(3, dtype=np.int64)), "s": pa.array(rows, pa.large_binary())})
    path = write(str(tmp_path / "l.arrows"), t)
    for expr, rows_kept in [(("s", "contains", needle), [0, 1]), (("s", "ends_with", needle), [1]),
                            (("s", "like", needle[:6] + b"%" + body[1000:1030] + b"%" + body[-30:]), [0]),
                            (("s", "like", b"%" + needle[:7] + b"%" + needle[7:]), [1]), (("s", "not like", b"%" + needle + b"%"), [2])]:
        assert check(con, path, t, expr, ["k"], compact=(False,)) == rows_kept
    assert check(con, path, t, ("s", "contains", needle), ["k"], compact=(True,)) == [0, 1]


# ----------------------------------------------------------------------------------------------- column types
WORDS = ["special", "requests", "Customer", "Complaints", "green", "BRASS", "furiously", "deposits", "ironic", "pending", "sleep", "quickly"]


def sentences(rng, n, p_null=0.05, lo=0, hi=6):
    pick = lambda: " ".join(WORDS[int(x)] for x in rng.integers(0, len(WORDS), int(rng.integers(lo, hi + 1))))
    return [None if rng.random() < p_null else pick() for _ in range(n)]


@pytest.fixture(scope="module")
def typed(tmp_path_factory):
    rng = np.random.default_rng(31)
    n = 9000
    s = sentences(rng, n)
    t = pa.table({
        "k": pa.array(np.arange(n, dtype=np.int64)),
        "ls": pa.array(s, pa.large_string()),
        "b": pa.array([None if v is None else v.encode() + (b"\x00\xff%_" if i % 3 else b"") for i, v in enumerate(s)], pa.binary()),
        "f3": pa.array([None if rng.random() < 0.1 else bytes(rng.integers(0, 3, 3, dtype=np.uint8)) for _ in range(n)], pa.binary(3)),
    })
    return write(str(tmp_path_factory.mktemp("typ") / "t.arrows"), t, max_chunksize=2500), t


TYPED_CASES = [("ls", "contains", "special"), ("ls", "like", "%special%requests%"), ("ls", "not like", "%special%requests%"), ("ls", "ends_with", "BRASS"),
               ("ls", "like", "%BRASS"), ("ls", "like", "green%green"), ("b", "contains", b"s\x00\xff"), ("b", "ends_with", b"BRASS\x00\xff%_"),
               ("b", "like", b"%Customer%Complaints%\xff%"), ("b", "contains", b"%_"), ("f3", "contains", b"\x00\x01"), ("f3", "ends_with", b"\x02"),
               ("f3", "like", b"\x01%\x01"), ("f3", "not like", b"%\x00%"), ("f3", "like", b"%\x02%\x02%\x02%")]


@pytest.mark.parametrize("expr", TYPED_CASES, ids=[str(e)[:60] for e in TYPED_CASES])
def test_large_string_binary_and_fixed_size_binary(con, typed, expr):
    path, t = typed
    check(con, path, t, expr, ["k", expr[0]])


DICT_CASES = [("author", "contains", "o"), ("author", "ends_with", "e"), ("author", "like", "%a%e%"), ("author", "not like", "%a%e%"),
              ("author", "like", "c%name"), ("author", "contains", "the third"),
              ("and", ("author", "not like", "%o%"), ("q", "<", 30)), ("or", ("author", "ends_with", "ob"), ("comp", "like", "%t%"))]


@pytest.mark.parametrize("expr", DICT_CASES, ids=[str(e)[:60] for e in DICT_CASES])
def test_dictionary_encoded_columns(con, tmp_path_factory, expr):
    """the dictionary is matched once per version on the host, with the header the kernel compiles; every record batch brings
    a replacement dictionary, entries and rows can be NULL"""
    rng = np.random.default_rng(8)
    n = 3000
    authors = ["alice", "bob", "carol the third of her name", "dave", None, "eve", ""]
    comps = ["C++", "Python", "Rust", "Go"]
    batches = []
    for bi in range(4):
        order = list(rng.permutation(len(authors)))
        a_vals = [authors[i] for i in order][: 4 + bi % 4]
        if None not in a_vals:
            a_vals[bi % len(a_vals)] = None                  # a NULL dictionary entry in every version
        a_idx = pa.array(rng.integers(0, len(a_vals), n).astype(np.int32), mask=rng.random(n) < 0.1)
        a = pa.DictionaryArray.from_arrays(a_idx, pa.array(a_vals, pa.string()))
        c_vals = comps[bi % 2:] + comps[: bi % 2]
        c = pa.DictionaryArray.from_arrays(pa.array(rng.integers(0, len(c_vals), n).astype(np.int8)), pa.array(c_vals, pa.large_string()))
        batches.append(pa.record_batch([pa.array(np.arange(bi * n, (bi + 1) * n, dtype=np.int64)), a, c,
                                        pa.array(rng.integers(0, 50, n).astype(np.int32))], names=["k", "author", "comp", "q"]))
    path = str(tmp_path_factory.mktemp("dct") / "d.arrows")
    with ipc.new_stream(path, batches[0].schema) as w:
        for b in batches:
            w.write_batch(b)
    t = pa.Table.from_batches(batches)
    # late materialisation with the row numbers alone: the dictionary column is then read by the filter only
    check(con, path, t, expr, ["k", "author"], compact=(False,), accept_dictionaries=True)
    check(con, path, t, expr, ["k"], compact=(True,), accept_dictionaries=True)
    cols, want = wanted(expr, t)
    assert con.read_arrow(path, accept_dictionaries=True).filter(expr).count(detail=True)["selected"] == len(want)
    if expr[1] == "not like":
        assert all(cols["author"][i] is not None for i in want)


def test_run_end_encoded_strings(con, tmp_path):
    rng = np.random.default_rng(5)
    runs = 2500
    values = sentences(rng, runs, p_null=0.1, lo=0, hi=5)
    lengths = rng.integers(1, 6, runs)
    ends = np.cumsum(lengths).astype(np.int32)
    n = int(ends[-1])
    ree = pa.RunEndEncodedArray.from_arrays(pa.array(ends), pa.array(values, pa.string()))
    flat = [v for v, c in zip(values, lengths) for _ in range(int(c))]
    t = pa.table({"k": pa.array(np.arange(n, dtype=np.int64)), "r": ree})
    path = write(str(tmp_path / "r.arrows"), t, max_chunksize=3000)
    flat_t = pa.table({"k": t.column("k"), "r": pa.array(flat, pa.string())})
    for expr in [("r", "contains", "special"), ("r", "like", "%special%requests%"), ("r", "not like", "%special%requests%"), ("r", "ends_with", "BRASS"),
                 ("and", ("r", "like", "%green%"), ("k", ">=", 100))]:
        check(con, path, flat_t, expr, ["k", "r"], compact=(False,))       # late materialisation refuses a run-end encoded column
        _, want = wanted(expr, flat_t)
        assert con.read_arrow(path, filter_compact=True).project(["k"]).filter(expr).fetch_columns()[0] == want


# ----------------------------------------------------------------------------------------------- trees and consumers
@pytest.fixture(scope="module")
def tpch(tmp_path_factory):
    rng = np.random.default_rng(77)
    n = 30000
    types = ["STANDARD POLISHED BRASS", "ECONOMY ANODIZED STEEL", "PROMO BRUSHED BRASS", "LARGE PLATED TIN", "SMALL BRASS COPPER"]
    t = pa.table({
        "k": pa.array(np.arange(n, dtype=np.int64)),
        "comment": pa.array(sentences(rng, n, p_null=0.04, lo=1, hi=8)),
        "ptype": pa.array([None if rng.random() < 0.03 else types[int(x)] for x in rng.integers(0, len(types), n)]),
        "size": pa.array(rng.integers(1, 51, n).astype(np.int32)),
        "price": pa.array(rng.random(n) * 1000.0, mask=rng.random(n) < 0.02),
        "mode": pa.array([["MAIL", "SHIP", "AIR", "RAIL"][int(x)] for x in rng.integers(0, 4, n)]),
    })
    d = tmp_path_factory.mktemp("tpch")
    return (write(str(d / "t.arrows"), t, max_chunksize=7000),
            write(str(d / "t_lz4.arrows"), t, max_chunksize=9000, options=ipc.IpcWriteOptions(compression="lz4")), t)


TREES = [
    ("and", ("comment", "not like", "%special%requests%"), ("size", "<", 25)),                                          # Q13
    ("and", ("comment", "like", "%Customer%Complaints%"), ("mode", "in", ["MAIL", "SHIP"])),                            # Q16
    ("and", ("ptype", "like", "%BRASS"), ("size", "=", 15)),                                                            # Q2
    ("and", ("comment", "like", "%green%"), ("price", "<", 500.0)),                                                     # Q9
    ("or", ("comment", "contains", "green special"), ("and", ("ptype", "ends_with", "TIN"), ("price", ">=", 900.0))),
    ("and", ("or", ("comment", "like", "%special%requests%"), ("size", "in", [1, 2, 3])), ("comment", "not like", "%green%"), ("ptype", "like", "%BRASS%")),
    ("or", ("and", ("comment", "like", "special%requests"), ("price", ">", 10.0)), ("comment", "is null"), ("ptype", "like", "LARGE%")),
]


@pytest.mark.parametrize("expr", TREES, ids=[str(e)[:70] for e in TREES])
def test_trees_mix_pattern_leaves_with_integer_float_and_in_leaves(con, tpch, expr):
    path, _, t = tpch
    before = da.filter_pattern_launches()
    want = check(con, path, t, expr, ["k", "comment", "size"])
    assert da.filter_pattern_launches() > before
    if expr == TREES[0]:
        comments = t.column("comment").to_pylist()
        assert all(comments[i] is not None for i in want)                 # NOT LIKE keeps no NULL row


def test_not_like_keeps_no_null_row(con, tpch):
    path, _, t = tpch
    for expr in [("comment", "not like", "%special%requests%"), ("comment", "not like", "special%"), ("comment", "not like", "special")]:
        cols, want = wanted(expr, t)
        assert t.column("comment").null_count > 100 and all(cols["comment"][i] is not None for i in want)
        check(con, path, t, expr, ["k", "comment"])


def test_consumers(con, tpch):
    """an LZ4 file (the filter reads the bytes the decompression kernels wrote), a device-resident consumer, and a count that
    does not project the filter column"""
    path, packed, t = tpch
    for expr in [("comment", "contains", "special"), ("and", ("comment", "like", "%special%requests%"), ("ptype", "ends_with", "BRASS"))]:
        _, want = wanted(expr, t)
        check(con, packed, t, expr, ["k", "comment"])
        for p in (path, packed):
            for kw in ({}, {"device_resident": True}):
                assert con.read_arrow(p, **kw).filter(expr).count(detail=True)["selected"] == len(want)
                assert con.read_arrow(p, **kw).project(["size"]).filter(expr).count(detail=True)["selected"] == len(want)


# ----------------------------------------------------------------------------------------------- folding and refusals
def test_folding_by_the_launch_counters(con, tpch):
    """A pattern without `%` is =, 'abc%' the prefix range, '%' IS NOT NULL: these run the base instance.  '%abc' is a pattern leaf."""
    path, _, t = tpch
    for expr in [("mode", "like", "MAIL"), ("mode", "like", "MA%"), ("mode", "like", "%"), ("mode", "not like", "MAIL"), ("mode", "not like", "MA%")]:
        base, ext = da.filter_launch_counts()
        pattern = da.filter_pattern_launches()
        check(con, path, t, expr, ["k", "mode"], degenerate=expr[2] == "%")
        assert da.filter_pattern_launches() == pattern and da.filter_launch_counts()[0] > base and da.filter_launch_counts()[1] == ext, expr
    counts = da.filter_launch_counts()
    pattern = da.filter_pattern_launches()
    check(con, path, t, ("mode", "like", "%AIL"), ["k", "mode"])
    assert da.filter_pattern_launches() > pattern and da.filter_launch_counts() == counts


def test_refusals(con, tpch, tmp_path):
    path, _, _ = tpch
    views = write(str(tmp_path / "v.arrows"), pa.table({"k": pa.array([1, 2, 3], pa.int64()), "sv": pa.array(["green", "blue", None], pa.string_view())}))
    nine = "%".join("abcdefghi")
    for p, expr in [(path, ("comment", "like", "a_c")), (path, ("comment", "not like", "%a_c%")), (path, ("comment", "like", nine)),
                    (path, ("size", "like", "%1%")), (path, ("size", "contains", "1")), (path, ("size", "ends_with", "1")), (path, ("size", "not like", "%1%")),
                    (views, ("sv", "contains", "ee")), (views, ("sv", "like", "%ee%")), (views, ("sv", "ends_with", "n"))]:
        with pytest.raises(da.MiError) as e:
            con.read_arrow(p).filter(expr).count()
        assert e.value.code == da._ffi.MI_ENOTSUP and "'%s'" % expr[0] in str(e.value), (expr, str(e.value))
    with pytest.raises(da.MiError) as e:
        con.read_arrow(path).filter(("comment", "like", "a_c")).count()
    assert "_" in str(e.value) and "UTF-8" in str(e.value)
    # eight segments are taken
    eight = "%" + "%".join("secarlnp") + "%"
    _, want = wanted(("comment", "like", eight), tpch[2])
    assert con.read_arrow(path).filter(("comment", "like", eight)).count() == len(want)
