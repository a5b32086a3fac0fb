"""The string leaves of the pushed-down filter -- leaf_strin (kLeafStrIn: = <> IN), strrow_compare / leaf_strrange (kLeafStrRange:
< <= > >= starts_with and LIKE 'p%'), leaf_dictmap (kLeafDictMap) and the host code in front of them (LeafOf's prefix successor,
DictMatchMap, the heap binding of BoundFilter::Program) -- at the byte, length, row-count and dictionary edges.

The values, the files and the expected rows come from tests/filter_string_cases.py: the evaluator there works on Python bytes
(byte-wise order, a proper prefix first, a comparison with NULL is not true) and is itself held against pyarrow.compute and
the oracle by tests/test_filter_string_reference_host.py, as is the string_t packer of the kernel-level tests.  Every scan
projects `k`, the row number, and the kept row numbers are compared exactly."""
import ctypes as C

import numpy as np
import pytest

import duckdb_arrow_amd as da
import filter_string_cases as sc
from duckdb_arrow_amd import _ffi

pytestmark = pytest.mark.gpu

ALL_COLUMNS = [n for names in sc.COLUMN_KINDS.values() for n in names]
BASE = sc.BASE


@pytest.fixture(scope="module")
def fx():
    return sc.fixture()


@pytest.fixture(scope="module")
def con():
    return da.Connection(0)


@pytest.fixture(scope="module")
def ctx():
    """the one context every kernel-level launch runs on"""
    c = da.Context(0)
    yield c
    c.close()


@pytest.fixture(scope="module")
def paths(fx, tmp_path_factory):
    d = tmp_path_factory.mktemp("filter_strings")
    out = {}
    for kind in sc.COLUMN_KINDS:
        out[kind] = str(d / (kind + ".arrows"))
        fx.write(out[kind], kind)
    for name in sc.COLUMN_KINDS["dict"]:   # and every dictionary column alone: a scan then decodes no other column's dictionaries
        out[name] = str(d / (name + ".arrows"))
        fx.write(out[name], "dict", names=[name])
    return out


# ---------------------------------------------------------------------------------------------------- kernel level
RESIDENT_ROWS = (1, 7, 8, 9, 63, 64, 65, 2047, 2048, 2049, 8191, 8192, 8193)
SENTINEL = -1


class ResidentVector:
    """a packed string_t vector in HBM, with a selection buffer one window longer than the kernel may write"""

    def __init__(self, ctx, values, layout, with_validity):
        import torch
        self.torch = torch
        self.ctx = ctx
        placement, self.ptr_base = sc.LAYOUTS[layout]
        self.n = len(values)
        images, heap, words = sc.pack_string_t(values, self.ptr_base, placement)
        # without validity words a NULL row's image is what it looks like: the empty string
        self.index = sc.index_values(values if with_validity else [b"" if v is None else v for v in values])
        self.rows = torch.from_numpy(images.reshape(-1).copy()).cuda()
        self.heap = torch.from_numpy(heap if len(heap) else np.zeros(8, np.uint8)).cuda()
        self.words = torch.from_numpy(words.view(np.int64)).cuda() if with_validity else None
        self.windows = (self.n + 2047) // 2048
        self.sel = torch.empty(((self.windows + 1) * 2048,), dtype=torch.int32, device="cuda")
        self.cnt = torch.empty((self.windows + 1,), dtype=torch.int32, device="cuda")

    def check(self, op, c):
        """one launch: the count and the first `count` entries of every window are the evaluator's, the slots behind them, the
        window past the end and its count still hold the sentinel"""
        torch = self.torch
        self.sel.fill_(SENTINEL)
        self.cnt.fill_(SENTINEL)
        torch.cuda.synchronize()   # the sentinels are in place before the kernel runs on the context's stream
        da.filter_string(self.ctx, self.rows.data_ptr(), self.words.data_ptr() if self.words is not None else 0, self.n, self.heap.data_ptr(),
                         self.ptr_base, op, c, self.sel.data_ptr(), self.cnt.data_ptr())
        sel_h, cnt_h = self.sel.cpu().numpy(), self.cnt.cpu().numpy()
        keep = sc.evaluate_indexed(self.index, op, c)
        what = (self.n, op, c)
        for w in range(self.windows):
            want = np.flatnonzero(keep[w * 2048: (w + 1) * 2048])
            assert cnt_h[w] == len(want), what + (w, "the kernel keeps %d rows, the evaluator %d" % (cnt_h[w], len(want)))
            assert np.array_equal(sel_h[w * 2048: w * 2048 + len(want)], want), what + (w,)
            assert (sel_h[w * 2048 + len(want): (w + 1) * 2048] == SENTINEL).all(), what + (w, "slots past the count were written")
        assert cnt_h[self.windows] == SENTINEL and (sel_h[self.windows * 2048:] == SENTINEL).all(), what
        return int(keep.sum())


@pytest.mark.parametrize("with_validity", [True, False], ids=["validity", "all_valid"])
@pytest.mark.parametrize("layout", list(sc.LAYOUTS))
def test_filter_string_every_pool_constant(fx, ctx, layout, with_validity):
    """mi_filter_string over 8193 rows of the binary pool: = <> < <= > >= starts_with against every pool value, its successor
    and its predecessor; the heap in Arrow order, shuffled with long strings at every address modulo 8, and under a pointer
    base that has nothing to do with where the heap lies"""
    vec = ResidentVector(ctx, fx.columns["binary"].values[:8193], layout, with_validity)
    for op in sc.OPS:
        kept = [vec.check(op, c) for c in sc.edge_constants(fx, "binary")]
        assert min(kept) + 50 < max(kept) and (max(kept) > 8193 // 2 or op == "="), op   # the constants separate the rows


@pytest.mark.parametrize("with_validity", [True, False], ids=["validity", "all_valid"])
@pytest.mark.parametrize("layout", list(sc.LAYOUTS))
def test_filter_string_at_every_row_count(fx, ctx, layout, with_validity):
    """1 .. 8193 rows, around a lane, a validity word, a window and a workgroup: '' (which the rows leaf_strin pads a window
    with equal), an inline, a 12-byte and a 13-byte constant, and one no row matches"""
    for n in RESIDENT_ROWS:
        values = list(fx.columns["binary"].values[:n])
        values[-1] = (b"", BASE[:13], BASE[:12], BASE[:4] + b"\x80")[n % 4]
        if n > 1:
            values[-2] = None if n % 2 else b""
        vec = ResidentVector(ctx, values, layout, with_validity)
        for op in sc.OPS:
            kept = [vec.check(op, c) for c in sc.reduced_constants()]
            if op == "=":
                assert kept[4] == 0 and (n < 2048 or min(kept[:4]) > 0)


# ---------------------------------------------------------------------------------------------------- scan level
def _int64_column(ch, i=0):
    if ch.size == 0:
        return np.zeros(0, np.int64)
    return np.ctypeslib.as_array(C.cast(ch.columns[i].data, C.POINTER(C.c_int64)), shape=(ch.size,))


def _selection(ch):
    return np.ctypeslib.as_array(ch.sel, shape=(ch.sel_count,)).astype(np.int64) if ch.sel_count else np.zeros(0, np.int64)


def _options(kind, options):
    return dict(options, accept_dictionaries=True) if kind == "dict" else options


def _kept(con, path, expr, **options):
    """the row numbers the scan keeps under `expr` (the filter columns are not projected)"""
    rel = con.read_arrow(path, **options).project(["k"]).filter(expr)
    try:
        out = [np.zeros(0, np.int64)]
        for ch in rel.chunks():
            k = _int64_column(ch)
            out.append(k[_selection(ch)] if ch.sel else k.copy())
        return np.concatenate(out)
    finally:
        rel.close()


def _counted(con, path, expr, **options):
    """(rows scanned, rows selected) of mi_scan_count with no column projected"""
    rel = con.read_arrow(path, **options).filter(expr)
    try:
        counted = rel.count(detail=True)
    finally:
        rel.close()
    return counted["rows"], counted["selected"]


def _kind(expr):
    kinds = {sc.kind_of(c) for c in sc._leaf_columns(expr) if c != "q"}
    assert len(kinds) == 1, expr
    return kinds.pop()


def _path(paths, expr):
    """the file of the columns' kind; a tree on one dictionary column reads the file that holds that column alone"""
    names = {c for c in sc._leaf_columns(expr) if c != "q"}
    return paths[names.pop()] if len(names) == 1 and _kind(expr) == "dict" else paths[_kind(expr)]


def _as_scan_sees(expr):
    """the evaluator's `not starts_with` is the scan's NOT LIKE 'p%'"""
    if not sc.is_leaf(expr):
        return (expr[0],) + tuple(_as_scan_sees(e) for e in expr[1:])
    return (expr[0], "not like", expr[2] + b"%") if expr[1] == "not starts_with" else expr


def _assert_rows(con, paths, fx, expr, scan_expr=None, **options):
    kind = _kind(expr)
    got = _kept(con, options.pop("path", None) or _path(paths, expr), _as_scan_sees(expr) if scan_expr is None else scan_expr, **_options(kind, options))
    want = np.flatnonzero(sc.evaluate(fx, expr))
    if not np.array_equal(got, want):
        missing, extra = np.setdiff1d(want, got), np.setdiff1d(got, want)
        raise AssertionError("%r %r: the scan keeps %d rows, the evaluator %d; first missing row %s, first row too many %s" % (
            scan_expr or expr, options, len(got), len(want), missing[:1].tolist(), extra[:1].tolist()))
    return len(want)


def _assert_values(con, paths, fx, expr, name):
    """the fetched keys and the fetched values of the filter column"""
    kind = _kind(expr)
    rel = con.read_arrow(_path(paths, expr), **_options(kind, {})).project(["k", name]).filter(expr)
    try:
        text = rel.types[1] == "VARCHAR"
        got_k, got_v = rel.fetch_columns()
    finally:
        rel.close()
    want = np.flatnonzero(sc.evaluate(fx, expr)).tolist()
    values = fx.columns[name].values
    assert got_k == want, expr
    assert got_v == [None if values[r] is None else (values[r].decode() if text else values[r]) for r in want], expr


@pytest.mark.parametrize("name", ALL_COLUMNS)
def test_every_op_at_every_edge_constant(con, paths, fx, name):
    """= <> < <= > >= starts_with against the column's own values, their successors and predecessors in byte order and members
    of every family of the pool; IS NULL and IS NOT NULL"""
    kept = [_assert_rows(con, paths, fx, leaf) for leaf in sc.single_leaf_cases(fx, name)]
    constants = sc.scan_constants(fx, name)
    for j, op in enumerate(sc.OPS):
        _assert_values(con, paths, fx, (name, op, constants[(j + 1) * len(constants) // 9]), name)
    if name == "dict_empty":
        assert sorted(set(kept)) == [0, sc.N_ROWS]   # IS NULL keeps everything, the rest nothing
    else:
        assert 0 in kept and max(kept) > sc.N_ROWS // 2 and sum(1 for n in kept if 0 < n < sc.N_ROWS - 1) > len(kept) // 2


@pytest.mark.parametrize("name", ALL_COLUMNS)
def test_in_lists(con, paths, fx, name):
    """empty, one value, duplicates, inline and long constants mixed, a tail family (equal length and prefix, different last
    1 .. 4 bytes), exactly 256 values; 257 are refused"""
    cases = sc.in_list_cases(fx, name)
    kept = [_assert_rows(con, paths, fx, leaf) for leaf in cases]
    assert {len(set(leaf[2])) for leaf in cases} >= {0, 1, 256} and kept[0] == 0
    _assert_values(con, paths, fx, cases[3], name)
    rel = con.read_arrow(paths.get(name, paths[sc.kind_of(name)]), **_options(sc.kind_of(name), {})).project(["k"])
    try:
        with pytest.raises(da.MiError, match="more than 256 values") as e:
            rel.filter(sc.too_long_in_list(name)).count()
    finally:
        rel.close()
    assert e.value.code == _ffi.MI_ENOTSUP


@pytest.mark.parametrize("name", ALL_COLUMNS)
def test_prefixes(con, paths, fx, name):
    """starts_with, LIKE 'p%' and NOT LIKE 'p%' with the prefixes '', ending in 0xFF, all 0xFF, 12 and 13 bytes long, a whole row
    and longer than every row: [p, successor(p)) with the trailing 0xFF bytes popped, no upper end when nothing is left; the
    negation keeps no NULL row"""
    nulls = sc.evaluate(fx, (name, "is null"))
    kept = []
    for p in sc.prefix_cases(fx, name):
        n = _assert_rows(con, paths, fx, (name, "starts_with", p))
        assert _assert_rows(con, paths, fx, (name, "starts_with", p), scan_expr=(name, "like", p + b"%")) == n
        m = _assert_rows(con, paths, fx, (name, "not starts_with", p))
        assert n + m == sc.N_ROWS - int(nulls.sum()) and not (sc.evaluate(fx, (name, "not starts_with", p)) & nulls).any()
        kept.append(n)
    assert kept[0] == sc.N_ROWS - int(nulls.sum()) and 0 in kept
    if name not in ("dict_empty", "fsb1", "fsb4", "fsb16"):
        assert sum(1 for n in kept if 0 < n < kept[0]) >= 4


@pytest.mark.parametrize("kind", list(sc.COLUMN_KINDS))
def test_generated_trees(con, paths, fx, kind):
    """seeded AND / OR trees of depth <= 3 with string leaves on two or three columns and integer leaves on q, at most 24
    leaves in conjunctive normal form, a quarter of them in need of distribution: accepted, and the rows of the tree as written"""
    trees = sc.generated_trees(fx, kind)
    assert len(trees) >= 40 and sum(sc.needs_distribution(t) for t in trees) >= 10
    kept = [_assert_rows(con, paths, fx, t) for t in trees]
    assert sum(1 for n in kept if 0 < n < sc.N_ROWS) >= 20


def test_a_tree_past_96_leaves_is_refused(con, paths):
    tree = sc.refused_tree()
    assert sc.cnf_size(tree)[1] > 96
    rel = con.read_arrow(paths["plain"]).project(["k"])
    try:
        with pytest.raises(da.MiError, match="too complex|leaves") as e:
            rel.filter(tree)
            assert rel.count() < 0   # never rows
    finally:
        rel.close()
    assert e.value.code == _ffi.MI_ENOTSUP


@pytest.mark.parametrize("name", sc.COLUMN_KINDS["dict"])
def test_dictionary_nulls(con, paths, fx, name):
    """a row is NULL through its index or through its dictionary entry: IS NULL keeps both, IS NOT NULL and <> neither, under
    every index type and under replaced, delta, empty and 300-entry dictionaries"""
    c = fx.columns[name]
    through_index = through_entry = 0
    for arr in c.arrays:
        through_index += arr.indices.null_count
        if arr.dictionary.null_count:
            entry_null = np.array([v is None for v in arr.dictionary.to_pylist()])
            through_entry += int(entry_null[np.array(arr.indices.drop_null().to_pylist(), np.int64)].sum())
    nulls = _assert_rows(con, paths, fx, (name, "is null"))
    assert nulls == through_index + through_entry and through_index > 0
    assert through_entry > 0 or name in ("dict_delta", "dict_empty")
    assert _assert_rows(con, paths, fx, (name, "is not null")) == sc.N_ROWS - nulls
    constant = (fx.index(name)[0] or [b"x"])[0]
    assert _assert_rows(con, paths, fx, (name, "<>", constant)) + _assert_rows(con, paths, fx, (name, "=", constant)) == sc.N_ROWS - nulls
    _assert_values(con, paths, fx, ("or", (name, "is null"), (name, ">=", constant)), name)


@pytest.mark.parametrize("kind", list(sc.COLUMN_KINDS))
def test_the_ways_a_chunk_is_delivered(con, paths, fx, tmp_path, kind):
    """selection vectors or compacted chunks (only `k` is projected then: a run-end encoded column may filter a compacted scan,
    not leave it), device-resident chunks, LZ4 and ZSTD bodies, the filter columns in or out of the projection, mi_scan_count"""
    expr = sc.delivery_cases()[kind]
    want = _assert_rows(con, paths, fx, expr)
    assert 100 < want < sc.N_ROWS - 100
    for name in dict.fromkeys(c for c in sc._leaf_columns(expr) if c != "q"):
        _assert_values(con, paths, fx, expr, name)
    assert _assert_rows(con, paths, fx, expr, filter_compact=True) == want
    for codec in ("lz4", "zstd"):
        packed = str(tmp_path / ("%s_%s.arrows" % (kind, codec)))
        fx.write(packed, kind, compression=codec)
        assert _assert_rows(con, paths, fx, expr, path=packed) == want
        for options in ({}, {"device_resident": True}):
            assert _counted(con, packed, expr, **_options(kind, options)) == (sc.N_ROWS, want), (codec, options)
    assert _counted(con, paths[kind], expr, **_options(kind, {"device_resident": True})) == (sc.N_ROWS, want)


def test_a_column_absent_from_one_file(con, paths, fx, tmp_path):
    """union_by_name over a file without the column: there every row is NULL -- a string leaf and its negation keep none of that
    file's rows, IS NULL all of them"""
    other = str(tmp_path / "without_binary.arrows")
    fx.write(other, "plain", names=[n for n in sc.COLUMN_KINDS["plain"] if n not in ("binary", "fsb13")])
    both = [paths["plain"], other]
    everything = np.arange(sc.N_ROWS)
    for name, c in (("binary", BASE[:12] + b"\x80"), ("fsb13", BASE[:13])):
        for expr in ((name, "=", c), (name, "<>", c), (name, ">=", b""), (name, "starts_with", b""), (name, "not like", c + b"%"),
                     (name, "in", [c, b""])):
            got = np.sort(_kept(con, both, expr, union_by_name=True))
            assert np.array_equal(got, np.flatnonzero(sc.evaluate(fx, expr if expr[1] != "not like" else (name, "not starts_with", c)))), expr
        got = np.sort(_kept(con, both, (name, "is null"), union_by_name=True))
        assert np.array_equal(got, np.sort(np.concatenate([np.flatnonzero(sc.evaluate(fx, (name, "is null"))), everything])))
        got = np.sort(_kept(con, both, ("or", (name, "=", c), ("q", ">=", 40)), union_by_name=True))
        q40 = np.flatnonzero(sc.evaluate(fx, ("q", ">=", 40)))
        assert np.array_equal(got, np.sort(np.concatenate([np.flatnonzero(sc.evaluate(fx, ("or", (name, "=", c), ("q", ">=", 40)))), q40])))


def _empty_dictionary_file(path, indices, nested, parent_mask=None):
    """k and a column whose dictionary has no entry, at the top level or as the child of a struct"""
    import pyarrow as pa
    import pyarrow.ipc as ipc
    column = pa.DictionaryArray.from_arrays(pa.array(indices, pa.int8()), pa.array([], pa.utf8()), safe=False)
    if nested:
        mask = None if parent_mask is None else pa.array(parent_mask, pa.bool_())
        column = pa.StructArray.from_arrays([column], names=["child"], mask=mask)
    batch = pa.record_batch([pa.array(np.arange(len(indices)), pa.int64()), column], names=["k", "nothing"])
    with ipc.new_stream(path, batch.schema) as w:
        w.write_batch(batch)


def _decoded_rows(con, path):
    rel = con.read_arrow(path, accept_dictionaries=True).project(["k", "nothing"])
    try:
        return sum(ch.size for ch in rel.chunks())
    finally:
        rel.close()


@pytest.mark.parametrize("where", ["top_level", "struct_child", "child_of_a_struct_with_nulls"])
def test_an_index_into_an_empty_dictionary_is_refused(con, tmp_path, where):
    """every row of a column whose dictionary is empty must be NULL (dict_empty above scans, and so does such a child of a
    struct); a valid index, 0 included, has nothing to point at and the decode refuses the file, whatever null count its
    metadata states and wherever the column stands.  The rows a tile is padded with are no such index."""
    nested = where != "top_level"
    parent_mask = [False, True, False, False, False] if where == "child_of_a_struct_with_nulls" else None   # True: a NULL struct
    path = str(tmp_path / "all_null.arrows")
    _empty_dictionary_file(path, [None] * 5, nested, parent_mask)
    assert _decoded_rows(con, path) == 5
    for j, index in enumerate((0, 5, 127)):
        indices = [None, None, None, None, None]
        indices[(0, 2, 4)[j]] = index
        path = str(tmp_path / ("broken%d.arrows" % j))
        _empty_dictionary_file(path, indices, nested, parent_mask)
        with pytest.raises(da.MiError, match="dictionary index out of range"):
            _decoded_rows(con, path)
