"""K6 on FLOAT / DOUBLE / HUGEINT / DECIMAL(19..38) columns: = <> < <= > >= IN and IS [NOT] NULL, alone and in AND / OR
trees with integer leaves, with selection vectors and with late materialisation, plain and dictionary-encoded.

The reference pushes no filters (filter_pushdown = false, src/scanner/read_arrow.cpp:47-48) and the oracle's CNF evaluator
knows integers only, so the yardstick is numpy over pyarrow's values with DuckDB's semantics written out here:
  * floating point is totally ordered: every NaN equals every other NaN (any sign, any payload), NaN is greater than every
    other value, +inf included, and -0.0 = +0.0;
  * a constant for a FLOAT column (Arrow float32, and float16 which the scan widens to FLOAT) is rounded to float32 first;
  * 128-bit integers compare as integers; a DECIMAL constant is its stored integer;
  * a NULL row passes no comparison.

The table has 2 x 2048 + 904 rows in two record batches of 3000 and 2000 rows: the first batch ends inside a window and the
last window of each batch is ragged; about 10 % of every column is NULL."""
import decimal
import math

import numpy as np
import pyarrow as pa
import pyarrow.ipc as ipc
import pytest

import duckdb_arrow_amd as da
from duckdb_arrow_amd import _ffi

pytestmark = pytest.mark.gpu

N = 2 * 2048 + 904
BATCH_ROWS = 3000
NAN = float("nan")
INF = float("inf")
P63, P64 = 1 << 63, 1 << 64
HUG_MAX, DEC25_MAX = 10 ** 38 - 1, 10 ** 25 - 1
WIDE_POOL = [0, 1, -1, 12345, P63 - 1, P63, P63 + 1, -P63, -P63 - 1, -P63 + 1, P64 - 1, P64, P64 + 1, -P64, -P64 - 1, -P64 + 1]
CTX = decimal.Context(prec=60)


@pytest.fixture(scope="module")
def con():
    return da.Connection(0)


def _float_column(rng, f, n):
    """quarters (so that constants like 1.5 are present and 1.3 is absent), a fifth of the rows special values"""
    u = {2: np.uint16, 4: np.uint32, 8: np.uint64}[np.dtype(f).itemsize]
    fi = np.finfo(f)
    vals = (np.round(rng.normal(0, 40, n)) / 4).astype(f)
    special = np.array([0.0, -0.0, fi.smallest_subnormal, -fi.smallest_subnormal, fi.tiny, -fi.tiny, fi.max, -fi.max, np.inf, -np.inf], f)
    bits = list(special.view(u))
    exp_all_ones = np.array([np.inf], f).view(u)[0]
    sign = u(1) << u(8 * np.dtype(f).itemsize - 1)
    quiet = u(1) << u(fi.nmant - 1)
    for payload in (quiet, u(1), quiet | u(0x12)):      # NaNs of both signs and three payloads
        bits += [exp_all_ones | payload, exp_all_ones | payload | sign]
    bits = np.array(bits, u)
    where = rng.random(n) < 0.2
    vals.view(u)[where] = bits[rng.integers(0, len(bits), int(where.sum()))]
    vals.view(u)[: len(bits)] = bits                    # every special value is there at least once
    return vals


def _wide_column(rng, n, most, bits):
    pool = WIDE_POOL + [most, -most]
    out = []
    for i in range(n):
        if i < len(pool):
            out.append(pool[i])
        elif rng.random() < 0.5:
            out.append(pool[int(rng.integers(0, len(pool)))])
        else:
            v = int(rng.integers(0, 1 << 62)) << (bits - 62) | int(rng.integers(0, 1 << 20))
            out.append(-v if rng.random() < 0.5 else v)
    return out


class Fixture:
    pass


@pytest.fixture(scope="module")
def fx(tmp_path_factory):
    rng = np.random.default_rng(77)
    f = Fixture()
    mask = lambda: rng.random(N) < 0.1
    f.floats = {"f32": _float_column(rng, np.float32, N), "f64": _float_column(rng, np.float64, N), "f16": _float_column(rng, np.float16, N)}
    f.wide = {"hug": _wide_column(rng, N, HUG_MAX, 120), "dec25": _wide_column(rng, N, DEC25_MAX, 80)}
    f.i32 = rng.integers(-50, 50, N).astype(np.int32)
    f.null = {name: mask() for name in ("f32", "f64", "f16", "hug", "dec25", "i32")}
    for name in f.null:
        f.null[name][:40] = False                       # the special values stay visible ...
        f.null[name][40:44] = True                      # ... and every column has NULL rows in the first window
    arrays = {"k": pa.array(np.arange(N, dtype=np.int64))}
    for name, vals in f.floats.items():
        arrays[name] = pa.array(vals, mask=f.null[name])
    arrays["hug"] = pa.array([None if m else decimal.Decimal(v) for v, m in zip(f.wide["hug"], f.null["hug"])], pa.decimal128(38, 0))
    arrays["dec25"] = pa.array([None if m else CTX.scaleb(decimal.Decimal(v), -3) for v, m in zip(f.wide["dec25"], f.null["dec25"])],
                               pa.decimal128(25, 3))
    arrays["i32"] = pa.array(f.i32, mask=f.null["i32"])
    table = pa.table(arrays)
    assert table.schema.field("f16").type == pa.float16() and table.num_rows == N
    f.path = str(tmp_path_factory.mktemp("fflt") / "t.arrows")
    with ipc.new_stream(f.path, table.schema) as w:
        w.write_table(table, max_chunksize=BATCH_ROWS)
    assert [b.num_rows for b in ipc.open_stream(f.path)] == [BATCH_ROWS, N - BATCH_ROWS]
    # what a scan hands back per column: floats as Python floats (float16 / float32 widened exactly), decimals as stored ints
    f.py = {"k": list(range(N)), "i32": [None if m else int(v) for v, m in zip(f.i32, f.null["i32"])]}
    for name, vals in f.floats.items():
        f.py[name] = [None if m else float(v) for v, m in zip(vals, f.null[name])]
    for name, vals in f.wide.items():
        f.py[name] = [None if m else v for v, m in zip(vals, f.null[name])]
    return f


# ------------------------------------------------------------------------------------------------ the yardstick
def _compare_float(v, op, c, is_float32):
    """DuckDB's total order on `v` (float32 or float64 values) against the constant c"""
    with np.errstate(over="ignore", invalid="ignore"):
        if is_float32:
            c = np.float32(c)                           # the constant is cast to the column's type
        vn, cn = np.isnan(v), bool(np.isnan(c))
        eq = (vn & cn) | (~vn & (not cn) & (v == c))    # IEEE == has -0.0 = +0.0
        lt = (~vn & cn) | (~vn & (not cn) & (v < c))    # NaN is the greatest
    gt = ~eq & ~lt
    return {"=": eq, "<>": ~eq, "<": lt, "<=": lt | eq, ">": gt, ">=": gt | eq}[op]


def _compare_int(v, op, c):
    fn = {"=": lambda x: x == c, "<>": lambda x: x != c, "<": lambda x: x < c, "<=": lambda x: x <= c, ">": lambda x: x > c,
          ">=": lambda x: x >= c}[op]
    return np.array([fn(x) for x in v], bool)


def _stored(c, column):
    """a Decimal constant as the integer a DECIMAL(25,3) column stores"""
    if isinstance(c, decimal.Decimal):
        assert column == "dec25"
        return int(CTX.scaleb(c, 3))
    return c


def _leaf(fx, column, op, c=None):
    ok = ~fx.null[column]
    if op == "is null":
        return ~ok
    if op == "is not null":
        return ok
    if column in fx.floats:
        v = fx.floats[column]
        v = v.astype(np.float32) if v.dtype == np.float16 else v          # the scan widens float16 to FLOAT
        cmp = lambda o, x: _compare_float(v, o, x, v.dtype == np.float32)
    else:
        v = fx.wide[column] if column in fx.wide else [int(x) for x in fx.i32]
        cmp = lambda o, x: _compare_int(v, o, _stored(x, column))
    if op == "in":
        m = np.zeros(N, bool)
        for x in c:
            m |= cmp("=", x)
    else:
        m = cmp(op, c)
    return m & ok                                       # a NULL row passes no comparison


def _evaluate(fx, e):
    if e[0] in ("and", "or") and isinstance(e[1], tuple):
        ms = [_evaluate(fx, kid) for kid in e[1:]]
        return np.logical_and.reduce(ms) if e[0] == "and" else np.logical_or.reduce(ms)
    return _leaf(fx, *e)


def _same(a, b):
    """value lists: NaN equals NaN, -0.0 differs from +0.0 (a scan returns the stored bits)"""
    norm = lambda x: "nan" if isinstance(x, float) and math.isnan(x) else (x, math.copysign(1.0, x)) if isinstance(x, float) else x
    return [norm(x) for x in a] == [norm(x) for x in b]


def _check(con, fx, expr, column, compact):
    want = np.flatnonzero(_evaluate(fx, expr)).tolist()
    # float16 is widened by a kernel that takes no selection vector: with late materialisation it can be a filter column,
    # not a projected one ("filter_compact needs flat projected columns")
    project = ["k"] if (compact and column == "f16") else ["k", column]
    got = con.read_arrow(fx.path, filter_compact=compact).project(project).filter(expr).fetch_columns()
    assert got[0] == want, expr
    if len(project) == 2:
        assert _same(got[1], [fx.py[column][i] for i in want]), expr
    return len(want)


# ------------------------------------------------------------------------------------------------ 1. every column, every op
FLOAT_CONSTANTS = [NAN, -0.0, INF, -INF, 1.5, 1.3, 65504.0, -5e-324]      # specials, present (1.5, float16's max), absent (1.3)
FLOAT_IN_LISTS = [[NAN, -0.0, 7.25], [1.3], [], [INF, -INF, 1.5, 2.5]]
WIDE_CONSTANTS = {   # extremes, values around +-2^63 and +-2^64, present and absent ones; those that fit travel as MI_FV_INT64
    "hug": [0, 12345, P63 - 1, -P63, P63, -P63 - 1, P64, -P64, HUG_MAX, -HUG_MAX, (1 << 127) - 1, -(1 << 127), (1 << 70) + 3],
    "dec25": [0, 12345, P63 - 1, -P63, P63, -P63 - 1, P64, -P64, DEC25_MAX, -DEC25_MAX, (1 << 70) + 3,
              decimal.Decimal("18446744073709551.616"), decimal.Decimal("-12.345")],
}
WIDE_IN_LISTS = [[0, P64, -P64 - 1], [P63, 7], [], [12345, -1, 1], [(1 << 70) + 3]]
COLUMNS = ["f32", "f64", "f16", "hug", "dec25"]
OPS = ["=", "<>", "<", "<=", ">", ">=", "in", "is null", "is not null"]


@pytest.mark.parametrize("compact", [False, True], ids=["sel", "compact"])
@pytest.mark.parametrize("op", OPS)
@pytest.mark.parametrize("column", COLUMNS)
def test_every_op_equals_numpy(con, fx, column, op, compact):
    """Every op meets NaN, -0.0 and NULL rows in the data; the floating-point ops also meet them as constants."""
    is_float = column in fx.floats
    if op in ("is null", "is not null"):
        exprs = [(column, op)]
    elif op == "in":
        exprs = [(column, op, vals) for vals in (FLOAT_IN_LISTS if is_float else WIDE_IN_LISTS)]
    else:
        exprs = [(column, op, c) for c in (FLOAT_CONSTANTS if is_float else WIDE_CONSTANTS[column])]
    kept = [_check(con, fx, e, column, compact) for e in exprs]
    assert max(kept) > 0                                # the case is not vacuous
    if is_float and op == "=":
        nan_rows = int((np.isnan(fx.floats[column]) & ~fx.null[column]).sum())
        zero_rows = int(((fx.floats[column] == 0) & ~fx.null[column]).sum())
        assert kept[0] == nan_rows >= 6 and kept[1] == zero_rows >= 2      # = NaN keeps every NaN, = -0.0 both zeros


# ------------------------------------------------------------------------------------------------ 2. mixed trees
TREES = [
    ("and", ("or", ("f64", ">", 2.5), ("i32", "in", [3, -7, 11])), ("dec25", "<=", P64)),
    ("and", ("or", ("f64", ">", NAN), ("i32", "in", [3, -7, 11])), ("dec25", "<=", decimal.Decimal("18446744073709551.616"))),
    ("and", ("f32", "<>", 1.5), ("hug", "<>", P63)),                                     # negated ranges
    ("and", ("f64", "<>", NAN), ("f64", "<>", -0.0), ("f64", ">=", -INF)),
    ("or", ("f16", "in", [NAN, -0.0, 0.25]), ("hug", "in", [P64, -P64, 0])),              # IN-lists with NaN and -0.0
    ("and", ("f64", ">", INF), ("f64", "<", INF)),                                       # keeps nothing: only NaN is > inf
    ("f64", ">=", NAN),                                                                  # keeps the NaN rows
    ("and", ("f32", ">", -INF), ("f32", "<", INF), ("f32", ">=", 0.0), ("f32", "<=", 10.50000001)),   # one merged range; 10.5 as float32
    ("and", ("hug", ">", -P64), ("hug", "<", P64), ("i32", "is not null")),
    ("or", ("and", ("f32", "<", 0.0), ("dec25", ">", 0)), ("and", ("f64", "is null"), ("hug", ">=", P63))),
]


@pytest.mark.parametrize("compact", [False, True], ids=["sel", "compact"])
@pytest.mark.parametrize("expr", TREES, ids=[str(e)[:60] for e in TREES])
def test_mixed_trees_equal_numpy(con, fx, expr, compact):
    want = np.flatnonzero(_evaluate(fx, expr)).tolist()
    got_k, got_f64, got_hug = con.read_arrow(fx.path, filter_compact=compact).project(["k", "f64", "hug"]).filter(expr).fetch_columns()
    assert got_k == want
    assert _same(got_f64, [fx.py["f64"][i] for i in want]) and got_hug == [fx.py["hug"][i] for i in want]
    # count without projecting the filter columns
    detail = con.read_arrow(fx.path).filter(expr).count(detail=True)
    assert (detail["rows"], detail["selected"]) == (N, len(want))


def test_empty_ranges(con, fx):
    assert con.read_arrow(fx.path).filter(("and", ("f64", ">", INF), ("f64", "<", INF))).count() == 0
    nan_rows = int((np.isnan(fx.floats["f64"]) & ~fx.null["f64"]).sum())
    assert con.read_arrow(fx.path).filter(("f64", ">=", NAN)).count() == nan_rows > 0
    assert con.read_arrow(fx.path).filter(("f64", ">", NAN)).count() == 0
    assert con.read_arrow(fx.path).filter(("hug", "<", -(1 << 127))).count() == 0


def test_more_than_one_workgroup_per_batch(con, tmp_path):
    """A workgroup takes four windows: 5 x 2048 + 5 rows in one record batch are two workgroups, the second one with a
    ragged window and three windows that do not exist."""
    n = 5 * 2048 + 5
    rng = np.random.default_rng(5)
    f64 = _float_column(rng, np.float64, n)
    wide = _wide_column(rng, n, HUG_MAX, 120)
    null = rng.random(n) < 0.1
    t = pa.table({"k": pa.array(np.arange(n, dtype=np.int64)), "f64": pa.array(f64, mask=null),
                  "hug": pa.array([None if m else decimal.Decimal(v) for v, m in zip(wide, null)], pa.decimal128(38, 0))})
    path = str(tmp_path / "big.arrows")
    with ipc.new_stream(path, t.schema) as w:
        w.write_table(t, max_chunksize=n)
    for compact in (False, True):
        want = np.flatnonzero(_compare_float(f64, "<=", -0.0, False) & ~null).tolist()
        assert con.read_arrow(path, filter_compact=compact).project(["k"]).filter(("f64", "<=", -0.0)).fetch_columns()[0] == want
        want = np.flatnonzero(_compare_int(wide, ">", P63) & ~null).tolist()
        assert con.read_arrow(path, filter_compact=compact).project(["k"]).filter(("hug", ">", P63)).fetch_columns()[0] == want


# ------------------------------------------------------------------------------------------------ 3. dictionary-encoded
DICT_EXPRS = [("d", op, c) for op in ("=", "<>", "<", "<=", ">", ">=") for c in (NAN, -0.0, 2.5, 1.3)] + [
    ("d", "in", [NAN, -0.0, 7.0]), ("d", "in", []), ("d", "is null"), ("d", "is not null"),
    ("and", ("or", ("d", ">", 0.0), ("q", "in", [1, 2])), ("d", "<>", INF)),
]


def test_dictionary_encoded_double_equals_its_plain_twin(con, tmp_path):
    """The dictionary leaf is evaluated once per dictionary version on the host, the rows by index; the second record batch
    brings a replacement dictionary, both have a NULL entry, and rows are NULL through their index too."""
    rng = np.random.default_rng(9)
    n = 2600
    dicts = [[1.5, NAN, None, -0.0, 2.5, INF, 0.0], [-INF, 2.5, None, -2.25, float.fromhex("-0x1.8p+1"), -NAN, 7.0, 1e-310]]
    batches, plain, nulls = [], [], []
    for bi, values in enumerate(dicts):
        idx = rng.integers(0, len(values), n).astype(np.int16)
        idx_null = rng.random(n) < 0.1
        d = pa.DictionaryArray.from_arrays(pa.array(idx, mask=idx_null), pa.array(values, pa.float64()))
        twin = [None if m or values[i] is None else values[i] for i, m in zip(idx, idx_null)]
        plain += twin
        batches.append(pa.record_batch([pa.array(np.arange(bi * n, (bi + 1) * n, dtype=np.int64)), d, pa.array(twin, pa.float64()),
                                        pa.array(rng.integers(0, 5, n).astype(np.int32))], names=["k", "d", "p", "q"]))
    path = str(tmp_path / "d.arrows")
    with ipc.new_stream(path, batches[0].schema) as w:
        for b in batches:
            w.write_batch(b)
    total = 2 * n
    null = np.array([v is None for v in plain])
    vals = np.array([0.0 if v is None else v for v in plain], np.float64)
    q = np.concatenate([b.column(3).to_numpy() for b in batches])

    def evaluate(e):
        if e[0] in ("and", "or") and isinstance(e[1], tuple):
            ms = [evaluate(kid) for kid in e[1:]]
            return np.logical_and.reduce(ms) if e[0] == "and" else np.logical_or.reduce(ms)
        if e[0] == "q":
            return np.isin(q, e[2])
        if e[1] in ("is null", "is not null"):
            return null if e[1] == "is null" else ~null
        if e[1] == "in":
            return np.logical_or.reduce([_compare_float(vals, "=", c, False) for c in e[2]] + [np.zeros(total, bool)]) & ~null
        return _compare_float(vals, e[1], e[2], False) & ~null

    def on_twin(e):
        if e[0] in ("and", "or") and isinstance(e[1], tuple):
            return (e[0],) + tuple(on_twin(kid) for kid in e[1:])
        return ("p" if e[0] == "d" else e[0],) + tuple(e[1:])

    for expr in DICT_EXPRS:
        want = np.flatnonzero(evaluate(expr)).tolist()
        got_k, got_d = con.read_arrow(path, accept_dictionaries=True).project(["k", "d"]).filter(expr).fetch_columns()
        twin_k, twin_p = con.read_arrow(path, accept_dictionaries=True).project(["k", "p"]).filter(on_twin(expr)).fetch_columns()
        assert got_k == twin_k == want, expr
        assert _same(got_d, twin_p) and _same(got_d, [plain[i] for i in want]), expr
        assert con.read_arrow(path, accept_dictionaries=True, filter_compact=True).project(["k"]).filter(expr).fetch_columns()[0] == want, expr


def test_float16_dictionary_replaced_then_extended_by_a_delta(con, tmp_path):
    """A float16 dictionary (widened to FLOAT on the host for the filter, on the device for the rows): 5 values, replaced by 65
    -- the extra NULL entry then lands in a new validity word -- and extended by a delta of 2, a record batch after each; a
    host consumer with a comparison pushed down on the column, against numpy over pyarrow's reading of the same file."""
    rng = np.random.default_rng(23)
    n = 2500
    first = np.array([1.5, -0.0, 65504.0, -np.inf, 0.25], np.float16)
    second = np.concatenate([np.array([0.0, -0.0, 6e-8, 6.104e-5, 65504.0, -65504.0, np.inf, -np.inf, 1.5], np.float16),
                             (np.arange(56) / 4 - 5).astype(np.float16)])
    third = np.concatenate([second, np.array([np.nan, 2.75], np.float16)])
    assert len(second) == 65 and len(third) == 67
    sch = pa.schema([("k", pa.int64()), ("d", pa.dictionary(pa.int16(), pa.float16()))])
    path = str(tmp_path / "f16_dict.arrows")
    with ipc.new_stream(path, sch, options=ipc.IpcWriteOptions(emit_dictionary_deltas=True)) as w:
        for bi, values in enumerate((first, second, third)):
            # the second entry of every dictionary is NULL, a tenth of the rows are NULL through their index
            d = pa.DictionaryArray.from_arrays(pa.array(rng.integers(0, len(values), n).astype(np.int16), mask=rng.random(n) < 0.1),
                                               pa.array(values, pa.float16(), mask=np.arange(len(values)) == 1))
            w.write_batch(pa.record_batch([pa.array(np.arange(bi * n, (bi + 1) * n, dtype=np.int64)), d], schema=sch))
    reader = ipc.open_stream(path)
    plain = reader.read_all().column("d").cast(pa.float16())
    assert reader.stats.num_dictionary_batches == 3 and reader.stats.num_replaced_dictionaries == 1 and reader.stats.num_dictionary_deltas == 1
    null = np.asarray(plain.is_null())
    vals = np.asarray(plain.fill_null(0)).astype(np.float32)
    py = [None if m else float(v) for v, m in zip(vals, null)]
    for expr in (("d", ">=", 1.5), ("d", "=", NAN), ("d", "<", 6.104e-5), ("d", "is null"), ("d", "in", [2.75, -0.0, 65504.0])):
        if expr[1] == "is null":
            mask = null
        elif expr[1] == "in":
            mask = np.logical_or.reduce([_compare_float(vals, "=", c, True) for c in expr[2]]) & ~null
        else:
            mask = _compare_float(vals, expr[1], expr[2], True) & ~null
        want = np.flatnonzero(mask).tolist()
        got_k, got_d = con.read_arrow(path, accept_dictionaries=True).project(["k", "d"]).filter(expr).fetch_columns()
        assert got_k == want and len(want) > 0, expr
        assert _same(got_d, [py[i] for i in want]), expr


# ------------------------------------------------------------------------------------------------ 4. errors
def _set_raw_filter(rel, column, value, value_kind):
    node = _ffi.FilterNode(op=_ffi.F_EQ, column=column.encode(), value=value, value_kind=value_kind)
    arr = (_ffi.FilterNode * 1)(node)
    _ffi.check(_ffi.lib().mi_scan_set_filter(rel._h, arr, 1, 0))


def test_constant_kinds_that_do_not_fit_the_column(con, fx, tmp_path):
    with pytest.raises(da.MiError, match="i32") as e:           # a double constant on an integer column
        con.read_arrow(fx.path).filter(("i32", "=", 1.5)).count()
    assert e.value.code == _ffi.MI_EINVAL
    with pytest.raises(da.MiError, match="f64") as e:           # an int constant on a DOUBLE column
        _set_raw_filter(con.read_arrow(fx.path), "f64", 1, _ffi.FV_INT64)
    assert e.value.code == _ffi.MI_EINVAL
    with pytest.raises(da.MiError, match="f32") as e:           # 128 bits on a FLOAT column
        _set_raw_filter(con.read_arrow(fx.path), "f32", 1, _ffi.FV_INT128)
    assert e.value.code == _ffi.MI_EINVAL
    with pytest.raises(da.MiError, match="i32") as e:           # 128 bits on a narrow column
        con.read_arrow(fx.path).filter(("i32", "=", 1 << 70)).count()
    assert e.value.code == _ffi.MI_EINVAL
    with pytest.raises(da.MiError, match="hug") as e:           # more digits than DECIMAL(38,0) has behind the point
        con.read_arrow(fx.path).filter(("hug", "=", decimal.Decimal("1.5"))).count()
    assert e.value.code == _ffi.MI_EINVAL
    # an interval column is still refused, in the words the integer path has always used
    t = pa.table({"k": pa.array(np.arange(10, dtype=np.int64)), "dur": pa.array(np.arange(10, dtype=np.int64), pa.duration("s"))})
    path = str(tmp_path / "dur.arrows")
    with ipc.new_stream(path, t.schema) as w:
        w.write_table(t)
    with pytest.raises(da.MiError, match="needs an integer") as e:
        con.read_arrow(path).filter(("dur", "=", 5)).count()
    assert e.value.code == _ffi.MI_ENOTSUP


# ------------------------------------------------------------------------------------------------ 5. which instance runs
def test_integer_programs_launch_the_instance_they_always_did(con, fx):
    """The kernel has two instances; only a program with a FLOAT / DOUBLE / 128-bit leaf launches the second one."""
    base0, ext0 = da.filter_launch_counts()
    assert con.read_arrow(fx.path).filter(("and", ("i32", ">", 0), ("k", "<", 4000))).count() > 0
    base1, ext1 = da.filter_launch_counts()
    assert base1 - base0 == 2 and ext1 == ext0              # one launch per record batch, all of the base instance
    assert con.read_arrow(fx.path).filter(("and", ("i32", ">", 0), ("f32", "<", 1.0))).count() > 0
    base2, ext2 = da.filter_launch_counts()
    assert base2 == base1 and ext2 - ext1 == 2
    assert con.read_arrow(fx.path).filter(("dec25", "is null")).count() > 0     # IS NULL needs no new code
    assert da.filter_launch_counts() == (base2 + 2, ext2)


# ------------------------------------------------------------------------------------------------ the one-leaf launch
@pytest.mark.parametrize("width", [4, 8, 16])
def test_filter_between_on_a_resident_vector(width):
    """mi_filter_between (what tools/filter_bench.py times): lo <= v <= hi on a vector in HBM, three workgroups, ragged."""
    import torch
    ctx = da.Context(0)
    n = 9 * 2048 + 77
    rng = np.random.default_rng(width)
    if width == 16:
        vals = _wide_column(rng, n, HUG_MAX, 120)
        host = np.array([[v & (P64 - 1), (v >> 64) & (P64 - 1)] for v in vals], np.uint64).view(np.int64)
        lo, hi = -P64, P63
        keep = _compare_int(vals, ">=", lo) & _compare_int(vals, "<=", hi)
    else:
        f = np.float32 if width == 4 else np.float64
        vals = _float_column(rng, f, n)
        host = vals.view(np.int32 if width == 4 else np.int64)
        lo, hi = -0.0, NAN
        keep = _compare_float(vals, ">=", lo, width == 4) & _compare_float(vals, "<=", hi, width == 4)
    dev = torch.from_numpy(host.copy()).cuda()
    sel = torch.full((n + 2048,), -1, dtype=torch.int32, device="cuda")
    cnt = torch.zeros((n + 2047) // 2048, dtype=torch.int32, device="cuda")
    da.filter_between(ctx, dev.data_ptr(), width, 0, n, lo, hi, sel.data_ptr(), cnt.data_ptr(), torch.cuda.current_stream().cuda_stream)
    torch.cuda.synchronize()
    cnt, sel = cnt.cpu().numpy(), sel.cpu().numpy()
    got = np.concatenate([w * 2048 + sel[w * 2048: w * 2048 + cnt[w]] for w in range(len(cnt))])
    assert got.tolist() == np.flatnonzero(keep).tolist() and len(got) > 0
    assert (sel[n:] == -1).all()                            # nothing is written past the last row
