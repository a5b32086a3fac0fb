"""The integer leaves of the pushed-down filter (leaf_compare<int8/16/32/64> with kLeafUnsigned / kLeafBias / kLeafNegate /
kLeafIn, and LeafOf, ToCnf, the range merge of NormaliseFilter and the uint64 mapping of BoundFilter::Program in front of
them) at the edges of every stored type and in record batches whose row counts are no multiple of 8.

The table and the expected rows come from tests/filter_integer_cases.py: the evaluator there works on the stored integers
in exact arithmetic and is itself held against the oracle by tests/test_filter_integer_reference_host.py.  Every scan projects
`k`, the row number, and the kept row numbers are compared exactly."""
import ctypes as C

import numpy as np
import pytest

import duckdb_arrow_amd as da
import filter_integer_cases as fc
from duckdb_arrow_amd import _ffi

pytestmark = pytest.mark.gpu

I64_MIN, I64_MAX, P63 = fc.I64_MIN, fc.I64_MAX, fc.P63


@pytest.fixture(scope="module")
def fx():
    return fc.fixture()


@pytest.fixture(scope="module")
def con():
    return da.Connection(0)


@pytest.fixture(scope="module")
def path(fx, tmp_path_factory):
    return fx.write(str(tmp_path_factory.mktemp("filter_integers") / "edges.arrows"))


def _int64_column(ch, i=0):
    if ch.size == 0:
        return np.zeros(0, np.int64)
    return np.ctypeslib.as_array(C.cast(ch.columns[i].data, C.POINTER(C.c_int64)), shape=(ch.size,))


def _selection(ch):
    return np.ctypeslib.as_array(ch.sel, shape=(ch.sel_count,)).astype(np.int64) if ch.sel_count else np.zeros(0, np.int64)


def _kept(con, path, expr, **options):
    """the row numbers the scan keeps under `expr`"""
    rel = con.read_arrow(path, **options).project(["k"]).filter(expr)
    try:
        out = [np.zeros(0, np.int64)]
        for ch in rel.chunks():
            k = _int64_column(ch)
            out.append(k[_selection(ch)] if ch.sel else k.copy())
        return np.concatenate(out)
    finally:
        rel.close()


def _want(fx, expr):
    return np.flatnonzero(fc.evaluate(fx, expr))


def _assert_rows(con, path, fx, expr, **options):
    got, want = _kept(con, path, expr, **options), _want(fx, expr)
    if not np.array_equal(got, want):
        missing, extra = np.setdiff1d(want, got), np.setdiff1d(got, want)
        raise AssertionError("%r %r: the scan keeps %d rows, the evaluator %d; first missing row %s, first row too many %s" % (
            expr, options, len(got), len(want), missing[:1].tolist(), extra[:1].tolist()))
    return len(want)


# ---------------------------------------------------------------------------------------------------- single leaves
@pytest.mark.parametrize("name", fc.filter_column_names())
def test_every_op_at_every_edge(con, path, fx, name):
    """= <> < <= > >= against the stored type's minimum - 1 .. maximum + 1, -1, 0, 1, INT64_MIN, INT64_MAX and the column's own
    extremes (constants outside the column's domain among them), IS NULL and IS NOT NULL"""
    kept = [_assert_rows(con, path, fx, leaf) for leaf in fc.single_leaf_cases(fx, name)]
    assert 0 in kept and max(kept) > fc.N_ROWS // 2


def test_uint64_above_int64_max_keeps_the_upper_half(con, path, fx):
    """`u64 > INT64_MAX` keeps the values >= 2^63 (the oracle's uv > uc); on every other column nothing is above INT64_MAX;
    `<>` keeps every valid row but INT64_MAX itself"""
    for name in ("u64", "u64_nn"):
        n = _assert_rows(con, path, fx, (name, ">", I64_MAX))
        assert n == int(((fx.stored[name] >= np.uint64(P63)) & fx.valid[name]).sum()) and n > 1000
        _assert_rows(con, path, fx, (name, "<>", I64_MAX))
        _assert_rows(con, path, fx, (name, ">=", I64_MAX))
        _assert_rows(con, path, fx, (name, "<=", I64_MAX))
    for name in ("i64", "i64_nn", "u32", "u8", "i8", "ts_us", "dec128_18", "flag"):
        assert _assert_rows(con, path, fx, (name, ">", I64_MAX)) == 0


# ---------------------------------------------------------------------------------------------------- IN-lists
def test_in_lists(con, path, fx):
    """empty, one value, duplicates, unsorted, outside the domain, negative on every unsigned width, exactly 256 values"""
    sizes = set()
    for leaf in fc.in_list_cases(fx):
        _assert_rows(con, path, fx, leaf)
        sizes.add(len(set(leaf[2])))
    assert {0, 1, 256} <= sizes


def test_negative_in_constants_never_match_an_unsigned_column(con, path, fx):
    """`u64 IN (-1, 5)` keeps the rows that hold 5, not those that hold 2^64 - 1; `u64 IN (-1, -2)` keeps nothing although
    2^64 - 1 and 2^64 - 2 are in the data"""
    for name in ("u64", "u64_nn"):
        v, ok = fx.stored[name], fx.valid[name]
        assert int(((v == np.uint64(2 ** 64 - 1)) & ok).sum()) > 300 and int(((v == np.uint64(2 ** 64 - 2)) & ok).sum()) > 300
        assert _assert_rows(con, path, fx, (name, "in", [-1, 5])) == int(((v == np.uint64(5)) & ok).sum()) > 100
        assert _assert_rows(con, path, fx, (name, "in", [-1, -2])) == 0
        assert _assert_rows(con, path, fx, (name, "in", [-2, I64_MIN, -1, 0, I64_MAX])) > 300
    for name in ("u8", "u16", "u32"):
        assert _assert_rows(con, path, fx, (name, "in", [-1, -2])) == 0
        assert _assert_rows(con, path, fx, (name, "in", [-1, 2])) > 300


def test_an_in_list_of_257_values_is_refused(con, path):
    rel = con.read_arrow(path).project(["k"])
    try:
        with pytest.raises(da.MiError, match="more than 256 values") as e:
            rel.filter(fc.too_long_in_list()).count()
    finally:
        rel.close()
    assert e.value.code == _ffi.MI_ENOTSUP


# ---------------------------------------------------------------------------------------------------- merge and trees
def test_range_merge(con, path, fx):
    """conjuncts on one column that fold into one range leaf (contradictions, INT64_MIN / INT64_MAX ends, negative bounds on
    uint64 columns, `> INT64_MAX` beside other ranges) and the forms that must not fold (<>, ranges under an OR)"""
    kept = [_assert_rows(con, path, fx, expr) for expr in fc.merge_cases(fx)]
    assert 0 in kept and max(kept) > 1000
    for name in ("u64", "u64_nn"):
        assert _assert_rows(con, path, fx, ("and", (name, ">=", 0), (name, "<", -1))) == 0
        assert _assert_rows(con, path, fx, ("and", (name, ">", I64_MAX), (name, ">=", 5))) > 1000
        assert _assert_rows(con, path, fx, ("and", (name, ">", -5), (name, "<", 10))) > 1000


def test_generated_trees(con, path, fx):
    """seeded AND / OR trees of depth <= 3 over all columns and leaf forms, at most 24 leaves in conjunctive normal form:
    every one is accepted and keeps the rows of the tree as written"""
    trees = fc.generated_trees(fx)
    assert len(trees) >= 40 and sum(fc.needs_distribution(t) for t in trees) >= 10
    assert all(fc.cnf_size(t)[1] <= 24 for t in trees)
    kept = [_assert_rows(con, path, fx, t) for t in trees]
    assert sum(1 for n in kept if 0 < n < fc.N_ROWS) >= 20   # (most trees are neither empty nor everything)


@pytest.mark.parametrize("tree", fc.refused_trees(), ids=["or_of_five_ands", "and_over_or_of_ands", "or_of_two_cnfs"])
def test_trees_past_96_leaves_are_refused(con, path, tree):
    assert fc.cnf_size(tree)[1] > 96
    rel = con.read_arrow(path).project(["k"])
    try:
        with pytest.raises(da.MiError, match="too complex|leaves") as e:
            rel.filter(tree)
            assert rel.count() < 0   # never rows
    finally:
        rel.close()
    assert e.value.code == _ffi.MI_ENOTSUP


def test_a_uint64_constant_past_int64_max_is_refused(con, path):
    """such a constant travels as MI_FV_INT128, which a narrow column does not take: MI_EINVAL naming the column"""
    for expr in (("u64", "=", P63), ("u64", ">", 2 ** 64 - 1), ("u64", "in", [1, P63])):
        rel = con.read_arrow(path).project(["k"])
        try:
            with pytest.raises(da.MiError, match="'u64'") as e:
                rel.filter(expr).count()
        finally:
            rel.close()
        assert e.value.code == _ffi.MI_EINVAL and "MI_FV_INT128" in str(e.value)


# ---------------------------------------------------------------------------------------------------- delivery
def _first_column(expr):
    return expr[0] if fc.is_leaf(expr) else _first_column(expr[1])


def _python_values(fx, name, rows):
    stored, ok = fx.stored[name], fx.valid[name]
    cast = bool if name.startswith("flag") else int
    return [cast(stored[r]) if ok[r] else None for r in rows]


@pytest.mark.parametrize("unset_all_valid", [False, True])
@pytest.mark.parametrize("zero_copy_direct", [None, False], ids=["alias", "materialised"])
@pytest.mark.parametrize("compact", [False, True])
def test_the_ways_a_chunk_is_delivered(con, path, fx, compact, zero_copy_direct, unset_all_valid):
    """selection vectors (ascending, chunk relative, sel_count rows) or compacted chunks, aliased or materialised vectors,
    validity words set or unset: the kept rows and their values are the evaluator's, and mi_scan_count and COUNT(*) agree"""
    options = dict(filter_compact=compact, zero_copy_direct=zero_copy_direct, unset_all_valid=unset_all_valid)
    for expr in fc.delivery_cases(fx):
        mask = fc.evaluate(fx, expr)
        want = np.flatnonzero(mask)
        name = _first_column(expr)
        rel = con.read_arrow(path, **options).project(["k", name]).filter(expr)
        try:
            seen = 0
            for ch in rel.chunks():
                if compact:
                    assert not ch.sel and ch.sel_count == ch.size, expr
                    assert np.array_equal(_int64_column(ch), want[seen: seen + ch.size]), expr
                    seen += ch.size
                    continue
                start = int(_int64_column(ch)[0])
                sel = _selection(ch)
                assert ch.sel and np.array_equal(sel, np.flatnonzero(mask[start: start + ch.size])), (expr, start)   # ascending, chunk relative
                seen += ch.sel_count
            assert seen == len(want), expr
        finally:
            rel.close()
        rel = con.read_arrow(path, **options).project(["k", name]).filter(expr)
        got_k, got_v = rel.fetch_columns()
        rel.close()
        assert got_k == want.tolist() and got_v == _python_values(fx, name, want), expr
        rel = con.read_arrow(path, **options).project(["k"]).filter(expr)
        counted = rel.count(detail=True)
        rel.close()
        assert (counted["rows"], counted["selected"]) == (fc.N_ROWS, len(want)), expr
        rel = con.read_arrow(path, **options).filter(expr)
        values, scanned, selected = rel.aggregate([("count_star",)], detail=True)
        rel.close()
        assert (values, scanned, selected) == ([len(want)], fc.N_ROWS, len(want)), expr


# ---------------------------------------------------------------------------------------------------- resident vectors
RESIDENT_ROWS = (1, 7, 8, 9, 63, 64, 65, 2047, 2048, 2049, 8191, 8192, 8193, 5 * 2048 + 5)


@pytest.mark.parametrize("with_validity", [True, False], ids=["validity", "all_valid"])
@pytest.mark.parametrize("width", [1, 2, 4, 8])
def test_filter_range_on_a_resident_vector(width, with_validity):
    """mi_filter_range (lo <= v < hi) over a vector in HBM at every row count around a lane, a word, a window and a workgroup:
    the count and the first `count` entries of every window, and nothing behind the last window's slot and the last count"""
    import torch
    ctx = da.Context(0)
    dtype = {1: np.int8, 2: np.int16, 4: np.int32, 8: np.int64}[width]
    lo_t, hi_t = int(np.iinfo(dtype).min), int(np.iinfo(dtype).max)
    bounds = [(lo_t, hi_t), (I64_MIN, I64_MAX), (1, 1), (-5, I64_MIN), (-1, 2)]
    rng = np.random.default_rng(100 * width + with_validity)
    stream = torch.cuda.current_stream().cuda_stream
    for n in RESIDENT_ROWS:
        pool = np.array(fc._edges(lo_t, hi_t), dtype)
        vals = pool[rng.integers(0, 7, n)]
        vals[-1] = hi_t if n % 2 else lo_t
        ok = rng.random(n) >= fc.NULL_FRACTION if with_validity else np.ones(n, bool)
        ok[-1] = True
        windows = (n + 2047) // 2048
        dev = torch.from_numpy(vals.copy()).cuda()
        words = torch.from_numpy(fc.validity_words(ok).view(np.int64)).cuda() if with_validity else None
        for lo, hi in bounds:
            sel = torch.full(((windows + 1) * 2048,), -1, dtype=torch.int32, device="cuda")
            cnt = torch.full((windows + 1,), -1, dtype=torch.int32, device="cuda")
            torch.cuda.synchronize()   # the sentinels are in place before the kernel runs, whatever stream it takes
            da.filter_range(ctx, dev.data_ptr(), width, words.data_ptr() if with_validity else 0, n, lo, hi, sel.data_ptr(), cnt.data_ptr(), stream)
            torch.cuda.synchronize()
            sel_h, cnt_h = sel.cpu().numpy(), cnt.cpu().numpy()
            v = vals.astype(np.int64)
            keep = ok & (v >= np.int64(lo)) & (v < np.int64(hi))
            what = (width, with_validity, n, lo, hi)
            for w in range(windows):
                want = np.flatnonzero(keep[w * 2048: (w + 1) * 2048])
                assert cnt_h[w] == len(want), what + (w,)
                assert np.array_equal(sel_h[w * 2048: w * 2048 + len(want)], want), what + (w,)
            assert cnt_h[windows] == -1 and (sel_h[windows * 2048:] == -1).all(), what
            if (lo, hi) in ((1, 1), (-5, I64_MIN)):
                assert not keep.any()
            if (lo, hi) == (I64_MIN, I64_MAX) and width == 8:
                assert keep.sum() == (ok & (vals != hi_t)).sum()   # the upper end is exclusive: an int64 maximum never passes


# ---------------------------------------------------------------------------------------------------- mi_scan_sum_product
@pytest.mark.parametrize("name", ["u8", "u16", "u32", "u64"])
def test_sum_product_refuses_unsigned_columns(con, path, fx, name):
    """agg_sum_product loads every value sign-extended (a uint16 60000 would count as -5536): an unsigned factor or filter
    column is MI_ENOTSUP, naming the column and mi_scan_aggregate, which handles unsigned columns"""
    for call in (lambda r: r.sum_product(name, "i32"), lambda r: r.sum_product("i32", name + "_nn"),
                 lambda r: r.sum_product("i16", "i32", [(name, 0, 5)])):
        rel = con.read_arrow(path)
        try:
            with pytest.raises(da.MiError, match="mi_scan_aggregate") as e:
                call(rel)
        finally:
            rel.close()
        assert e.value.code == _ffi.MI_ENOTSUP and ("'%s'" % name in str(e.value) or "'%s_nn'" % name in str(e.value))
    # ... which gives the unsigned sum
    rel = con.read_arrow(path).filter(("i16", "is not null"))
    got = rel.aggregate([("sum_product", name, "i8_nn")])
    rel.close()
    keep = fx.valid["i16"] & fx.valid[name]
    want = sum(int(a) * int(b) for a, b in zip(fx.stored[name][keep], fx.stored["i8_nn"][keep]))
    assert got == [(want + (1 << 127)) % (1 << 128) - (1 << 127)]


@pytest.mark.parametrize("a,b", [("i8", "i16"), ("i16", "i32"), ("i32", "i64"), ("i64", "i8"), ("i64", "ts_us")])
def test_sum_product_over_signed_columns_stays_exact(con, path, fx, a, b):
    """every signed width as a factor, over ragged record batches (8197, 2047, 0, 1, ... rows) with NULLs in the filter columns
    and in both factors: the 128-bit sum (modulo 2^128, as documented) and the selected rows are exact"""
    filters = [("date64", -1, 2), ("i32", I64_MIN, 2)]
    keep = np.ones(fc.N_ROWS, bool)
    for f, lo, hi in filters:
        v = fx.stored[f].astype(np.int64)
        keep &= fx.valid[f] & (v >= np.int64(lo)) & (v < np.int64(hi))
    assert not fx.valid[a].all() and not fx.valid[b].all() and not fx.valid["date64"].all()
    both = keep & fx.valid[a] & fx.valid[b]
    want = sum(int(x) * int(y) for x, y in zip(fx.stored[a][both], fx.stored[b][both]))
    rel = con.read_arrow(path)
    total, selected, scanned = rel.sum_product(a, b, filters)
    rel.close()
    assert (selected, scanned) == (int(keep.sum()), fc.N_ROWS) and selected > 1000
    assert total == (want + (1 << 127)) % (1 << 128) - (1 << 127)
    if (a, b) == ("i32", "i64"):
        assert abs(want) > 2 ** 64   # beyond 64 bits
