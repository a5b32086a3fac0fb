"""mi_scan_aggregate through the scan: SELECT agg_1 .. agg_n WHERE <pushed-down filter>, against Python integers, math.fsum
and pyarrow's reading of the same file.  Expected values never come from the library.

The table has 23 000 rows in record batches of 7000 (several windows per batch, ragged last windows, more batches than the
three pipeline slots), one column of every value class, 10 - 20 % NULLs.  One column is dictionary-encoded, so every scan of the
file sets accept_dictionaries (a stream that holds a DictionaryBatch is refused without it, whatever is projected).  Float sums are held to the bound of any summation
order, |err| <= 2 n 2^-53 sum|x_i| (see test_gpu_aggregate_vectors.py); everything else is exact."""
import datetime
import decimal
import math
import os
import struct

import numpy as np
import pyarrow as pa
import pyarrow.compute as pc
import pyarrow.ipc as ipc
import pytest

import duckdb_arrow_amd as da
from duckdb_arrow_amd import _ffi

pytestmark = pytest.mark.gpu

N = 23000
BATCH_ROWS = 7000
CTX = decimal.Context(prec=60)
EPOCH = datetime.date(1970, 1, 1)
CANONICAL_NAN = 0x7FF8000000000000
MODES = [dict(device_resident=True), dict(), dict(device_resident=True, unset_all_valid=True, zero_copy_direct=True),
         dict(unset_all_valid=True, zero_copy_direct=False)]
WORDS = ["special", "regular", "express", "pending", "final", "ironic", "bold", "quick packages", "carefully special requests", ""]
MODES_OF_SHIP = ["MAIL", "SHIP", "RAIL", "AIR", "TRUCK", "REG AIR", "FOB"]


@pytest.fixture(scope="module")
def con():
    return da.Connection(0)


def _stored(v, t):
    """a pyarrow value as the scan stores it: DECIMAL -> the unscaled integer, DATE -> days, floats widened"""
    if v is None:
        return None
    if pa.types.is_decimal(t):
        return int(CTX.scaleb(v, t.scale))
    if pa.types.is_date32(t):
        return (v - EPOCH).days
    if pa.types.is_floating(t):
        return float(v)
    return v


def _read_back(path):
    table = ipc.open_stream(path).read_all()
    out = {}
    for name in table.column_names:
        col = table.column(name)
        t = col.type
        if pa.types.is_dictionary(t):
            col, t = col.cast(t.value_type), t.value_type
        if isinstance(t, pa.RunEndEncodedType):
            vt = t.value_type
            out[name] = [_stored(v, vt) for chunk in col.chunks for v in pc.run_end_decode(chunk).to_pylist()]
            continue
        if t == pa.float16():
            out[name] = [None if v is None else float(v) for v in col.to_pylist()]
            continue
        out[name] = [_stored(v, t) for v in col.to_pylist()]
    return out


class Fixture:
    pass


@pytest.fixture(scope="module")
def fx(tmp_path_factory):
    rng = np.random.default_rng(4242)
    mask = lambda: rng.random(N) < rng.uniform(0.10, 0.20)
    arrays = {"k": pa.array(np.arange(N, dtype=np.int64))}
    for name, t in (("i8", np.int8), ("i16", np.int16), ("i32", np.int32), ("i64", np.int64), ("u8", np.uint8), ("u16", np.uint16),
                    ("u32", np.uint32), ("u64", np.uint64)):
        info = np.iinfo(t)
        v = rng.integers(info.min, info.max, N, dtype=t, endpoint=True)
        v[:3] = [info.min, info.max, info.max]
        arrays[name] = pa.array(v, mask=mask())
    arrays["f32"] = pa.array(rng.normal(0, 100, N).astype(np.float32), mask=mask())
    arrays["f64"] = pa.array(rng.normal(0, 1e4, N) * rng.choice([1e-6, 1.0, 1e6], N), mask=mask())
    arrays["f16"] = pa.array((np.round(rng.normal(0, 40, N)) / 4).astype(np.float16), mask=mask())
    m = mask()
    arrays["dec"] = pa.array([None if x else CTX.scaleb(decimal.Decimal(int(v)), -2) for v, x in zip(rng.integers(-10 ** 14, 10 ** 14, N), m)],
                             pa.decimal128(15, 2))
    arrays["date"] = pa.array(rng.integers(8000, 11000, N).astype(np.int32), pa.int32(), mask=mask()).cast(pa.date32())
    m = mask()
    hug = [(int(rng.integers(0, 1 << 62)) << int(rng.integers(0, 60))) * (-1 if rng.random() < 0.5 else 1) for _ in range(N)]
    arrays["hug"] = pa.array([None if x else decimal.Decimal(v) for v, x in zip(hug, m)], pa.decimal128(38, 0))
    m = mask()
    arrays["s"] = pa.array([None if x else MODES_OF_SHIP[i] for i, x in zip(rng.integers(0, len(MODES_OF_SHIP), N), m)], pa.string())
    m = mask()
    arrays["c"] = pa.array([None if x else " ".join(WORDS[j] for j in rng.integers(0, len(WORDS), 3)) for x in m], pa.string())
    m = mask()
    arrays["d"] = pa.array([None if x else MODES_OF_SHIP[i] for i, x in zip(rng.integers(0, len(MODES_OF_SHIP), N), m)], pa.string()).dictionary_encode()
    arrays["b"] = pa.array(rng.random(N) < 0.5, mask=mask())
    m = mask()
    arrays["lst"] = pa.array([None if x else list(range(i % 4)) for i, x in enumerate(m)], pa.list_(pa.int32()))
    m = mask()
    arrays["st"] = pa.array([None if x else {"x": i, "y": str(i)} for i, x in enumerate(m)], pa.struct([("x", pa.int64()), ("y", pa.string())]))
    table = pa.table(arrays)
    f = Fixture()
    f.path = str(tmp_path_factory.mktemp("agg") / "t.arrows")
    with ipc.new_stream(f.path, table.schema) as w:
        w.write_table(table, max_chunksize=BATCH_ROWS)
    assert [b.num_rows for b in ipc.open_stream(f.path)] == [7000, 7000, 7000, 2000]
    f.py = _read_back(f.path)
    assert all(0.08 * N < sum(v is None for v in f.py[c]) < 0.22 * N for c in f.py if c != "k")
    return f


NUMERIC = ["i8", "i16", "i32", "i64", "u8", "u16", "u32", "u64", "f32", "f64", "f16", "dec", "date"]
FLOATS = {"f32", "f64", "f16"}


def all_specs():
    specs = [("count_star",)]
    for c in NUMERIC:
        specs += [("count", c), ("sum", c), ("min", c), ("max", c)]
    specs += [("count", "hug"), ("min", "hug"), ("max", "hug"), ("count", "s"), ("count", "c"), ("count", "lst"), ("count", "st"), ("count", "b")]
    specs += [("sum_product", "i64", "i32"), ("sum_product", "u64", "i8"), ("sum_product", "dec", "date"), ("sum_product", "u32", "u32"),
              ("sum_product", "f32", "f64"), ("sum_product", "f16", "f16"), ("sum_product", "i16", "u64")]
    return specs


def _wrap128(v):
    v &= (1 << 128) - 1
    return v - (1 << 128) if v >> 127 else v


def _bits(x):
    return struct.unpack("<Q", struct.pack("<d", x))[0]


def _float_key(x):
    return (1, 0.0) if math.isnan(x) else (0, x + 0.0)


def expected(py, spec, rows):
    op, cols = spec[0], spec[1:]
    if op == "count_star":
        return "exact", len(rows)
    rows = [r for r in rows if all(py[c][r] is not None for c in cols)]
    if op == "count":
        return "exact", len(rows)
    if not rows:
        return "exact", None
    vals = [py[cols[0]][r] for r in rows]
    if op == "sum_product":
        vals = [x * py[cols[1]][r] for x, r in zip(vals, rows)]
    if cols[0] in FLOATS:
        if op in ("sum", "sum_product"):
            return "sum", vals
        best = (min if op == "min" else max)(vals, key=_float_key)
        return "exact", float("nan") if math.isnan(best) else best + 0.0
    if op in ("sum", "sum_product"):
        return "exact", _wrap128(sum(vals))
    return "exact", (min if op == "min" else max)(vals)


def check(got, want, what):
    kind, value = want
    if kind == "sum":
        exact = math.fsum(value)
        bound = 2 * len(value) * 2.0 ** -53 * math.fsum(abs(v) for v in value)
        assert isinstance(got, float) and abs(got - exact) <= bound, (what, got, exact, bound)
    elif isinstance(value, float):
        assert isinstance(got, float) and _bits(got) == (CANONICAL_NAN if math.isnan(value) else _bits(value)), (what, got, value)
    else:
        assert got == value and (value is None or isinstance(got, int)), (what, got, value)


def aggregate_all(rel_factory, specs):
    """every spec, 8 to a call (a scan each) -> values, and the (scanned, selected) of every call"""
    values, seen = [], set()
    for first in range(0, len(specs), 8):
        v, scanned, selected = rel_factory().aggregate(specs[first: first + 8], detail=True)
        values += v
        seen.add((scanned, selected))
    return values, seen


def _like(pattern_parts):
    """rows that hold the parts in order (a %-pattern with % at both ends)"""
    def match(v):
        at = 0
        for p in pattern_parts:
            at = v.find(p, at)
            if at < 0:
                return False
            at += len(p)
        return True
    return match


FILTERS = {
    "none": (None, lambda py, r: True, {}),
    "integer range": (("and", ("i32", ">=", -(1 << 30)), ("i32", "<", 1 << 30)), lambda py, r: py["i32"][r] is not None and -(1 << 30) <= py["i32"][r] < (1 << 30), {}),
    "float leaf": (("f32", ">", 12.5), lambda py, r: py["f32"][r] is not None and py["f32"][r] > 12.5, {}),
    "128-bit leaf": (("hug", "<", 1 << 70), lambda py, r: py["hug"][r] is not None and py["hug"][r] < (1 << 70), {}),
    "string in": (("s", "in", ["MAIL", "SHIP"]), lambda py, r: py["s"][r] in ("MAIL", "SHIP"), {}),
    "starts_with": (("c", "starts_with", "spec"), lambda py, r: py["c"][r] is not None and py["c"][r].startswith("spec"), {}),
    "like": (("c", "like", "%special%req%"), lambda py, r: py["c"][r] is not None and _like(["special", "req"])(py["c"][r]), {}),
    "or of two columns": (("or", ("i16", "<", -20000), ("f64", ">", 1e3)),
                          lambda py, r: (py["i16"][r] is not None and py["i16"][r] < -20000) or (py["f64"][r] is not None and py["f64"][r] > 1e3), {}),
    "dictionary column": (("d", "=", "RAIL"), lambda py, r: py["d"][r] == "RAIL", {}),
    "column that is not aggregated": (("k", "<", 9001), lambda py, r: r < 9001, {}),
}


@pytest.mark.parametrize("name", list(FILTERS))
def test_every_operation_under_every_filter_form(con, fx, name):
    expr, keep, extra = FILTERS[name]
    rows = [r for r in range(N) if keep(fx.py, r)]
    assert 0 < len(rows) <= N and (expr is None or len(rows) < N)
    specs = all_specs()
    want = [expected(fx.py, sp, rows) for sp in specs]
    for mode in MODES:
        def make():
            rel = con.read_arrow(fx.path, accept_dictionaries=True, **dict(mode, **extra))
            return rel.filter(expr) if expr is not None else rel
        got, seen = aggregate_all(make, specs)
        assert seen == {(N, len(rows))}, (name, mode, seen)
        for sp, g, w in zip(specs, got, want):
            check(g, w, (name, mode, sp))


def test_filter_compact_is_ignored_and_filter_range_is_honoured(con, fx):
    rows = [r for r in range(N) if fx.py["i32"][r] is not None and -5000 <= fx.py["i32"][r] < (1 << 29)]
    specs = [("sum", "i64"), ("count", "c"), ("min", "f64"), ("count_star",)]
    want = [expected(fx.py, sp, rows) for sp in specs]
    for compact in (False, True):
        rel = con.read_arrow(fx.path, accept_dictionaries=True, filter_compact=compact, device_resident=True).filter_range("i32", -5000, 1 << 29)
        got, scanned, selected = rel.aggregate(specs, detail=True)
        assert (scanned, selected) == (N, len(rows))
        for sp, g, w in zip(specs, got, want):
            check(g, w, sp)


def test_q6_with_the_predicates_given_through_filter(con):
    """the known answer test_q6_fused_on_the_gpu_known_answer pins, by the general form, and its neighbours from pyarrow"""
    path = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "lineitem_sf0_01_q6.arrows")
    py = _read_back(path)
    n = len(py["l_shipdate"])
    rows = [r for r in range(n) if 8766 <= py["l_shipdate"][r] < 9131 and 5 <= py["l_discount"][r] < 8 and py["l_quantity"][r] < 2400]
    q6 = ("and", ("l_shipdate", ">=", 8766), ("l_shipdate", "<", 9131), ("l_discount", ">=", 5), ("l_discount", "<", 8), ("l_quantity", "<", 2400))
    specs = [("sum_product", "l_extendedprice", "l_discount"), ("count_star",), ("min", "l_shipdate"), ("max", "l_shipdate"), ("sum", "l_quantity")]
    got, scanned, selected = con.read_arrow(path).filter(q6).aggregate(specs, detail=True)
    assert got[0] == 11930532253 and selected == 1191 and scanned == n
    old = con.read_arrow(path).sum_product("l_extendedprice", "l_discount", [("l_shipdate", 8766, 9131), ("l_discount", 5, 8), ("l_quantity", -2 ** 63, 2400)])
    assert old == (got[0], selected, scanned)
    assert got[1:] == [len(rows), min(py["l_shipdate"][r] for r in rows), max(py["l_shipdate"][r] for r in rows), sum(py["l_quantity"][r] for r in rows)]
    assert got[0] == sum(py["l_extendedprice"][r] * py["l_discount"][r] for r in rows)


def test_run_end_encoded_column(con, tmp_path):
    rng = np.random.default_rng(8)
    n, per_batch = 9000, 4500
    path = str(tmp_path / "ree.arrows")
    schema = pa.schema([("r", pa.run_end_encoded(pa.int32(), pa.int64())), ("k", pa.int64())])
    with ipc.new_stream(path, schema) as w:
        for first in range(0, n, per_batch):                      # two record batches, each with run ends of its own
            ends = np.cumsum(rng.integers(1, 40, 400))
            ends = ends[ends < per_batch].tolist() + [per_batch]
            values = [None if rng.random() < 0.15 else int(v) for v in rng.integers(-10 ** 12, 10 ** 12, len(ends))]
            ree = pa.RunEndEncodedArray.from_arrays(pa.array(ends, pa.int32()), pa.array(values, pa.int64()))
            w.write_batch(pa.record_batch([ree, pa.array(np.arange(first, first + per_batch, dtype=np.int64))], schema=schema))
    py = _read_back(path)
    assert len(py["r"]) == n and any(v is None for v in py["r"])
    specs = [("sum", "r"), ("min", "r"), ("count", "r"), ("max", "r"), ("count_star",)]
    for expr, rows in ((None, list(range(n))), (("k", ">=", 2500), list(range(2500, n))), (("r", "<", 0), [r for r in range(n) if py["r"][r] is not None and py["r"][r] < 0])):
        for mode in MODES:
            rel = con.read_arrow(path, **mode)
            got = (rel.filter(expr) if expr else rel).aggregate(specs)
            for sp, g in zip(specs, got):
                check(g, expected(py, sp, rows), (expr, mode, sp))


def test_two_contexts_and_rank_world_merge_to_the_unsharded_results(con, fx):
    specs = [("count_star",), ("sum", "i64"), ("min", "hug"), ("max", "f32"), ("sum", "f64"), ("count", "lst"), ("sum_product", "u64", "i8"), ("min", "u64")]
    expr = ("c", "like", "%special%")
    rows = [r for r in range(N) if fx.py["c"][r] is not None and "special" in fx.py["c"][r]]
    want = [expected(fx.py, sp, rows) for sp in specs]
    runs = []
    for _ in range(2):
        rel = con.read_arrow(fx.path, accept_dictionaries=True, contexts=[da.Context(0), da.Context(0)], device_resident=True).filter(expr)
        got, scanned, selected = rel.aggregate(specs, detail=True)
        assert (scanned, selected) == (N, len(rows))
        for sp, g, w in zip(specs, got, want):
            check(g, w, ("two contexts", sp))
        runs.append(got)
    assert _bits(runs[0][4]) == _bits(runs[1][4]) and runs[0] == runs[1]       # the two-context double sum is bit-reproducible
    # rank / world = 2: each rank returns its share -- COUNT and SUM add up, MIN and MAX merge
    parts = [con.read_arrow(fx.path, accept_dictionaries=True, rank=r, world=2).filter(expr).aggregate(specs, detail=True) for r in range(2)]
    assert sum(p[1] for p in parts) == N and sum(p[2] for p in parts) == len(rows)
    a, b = parts[0][0], parts[1][0]
    assert a[0] + b[0] == want[0][1] and a[1] + b[1] == want[1][1] and a[5] + b[5] == want[5][1] and _wrap128(a[6] + b[6]) == want[6][1]
    assert min(a[2], b[2]) == want[2][1] and max(a[3], b[3]) == want[3][1] and min(a[7], b[7]) == want[7][1]
    check(a[4] + b[4], ("sum", want[4][1] + [0.0]), "rank sums add up")         # one more addition: n + 1 terms in the bound


def test_refusals_name_the_column_and_the_operation(con, fx):
    def refused(specs, code, *words, **options):
        rel = con.read_arrow(fx.path, accept_dictionaries=True, **options)
        try:
            with pytest.raises(da.MiError) as e:
                rel.aggregate(specs)
        finally:
            rel.close()      # (a traceback keeps its frames' relations in a reference cycle: closed here, not by the cycle collector)
        assert e.value.code == code, (specs, e.value.code, str(e.value))
        for w in words:
            assert w in str(e.value), (specs, w, str(e.value))

    refused([("sum", "s")], _ffi.MI_ENOTSUP, "'s'", "SUM", "VARCHAR")
    refused([("min", "b")], _ffi.MI_ENOTSUP, "'b'", "MIN", "BOOLEAN")
    refused([("sum", "hug")], _ffi.MI_ENOTSUP, "'hug'", "SUM")
    refused([("max", "lst")], _ffi.MI_ENOTSUP, "'lst'", "MAX")
    refused([("sum_product", "i32", "f64")], _ffi.MI_ENOTSUP, "'i32'", "'f64'", "SUM_PRODUCT")
    refused([("sum_product", "f32", "dec")], _ffi.MI_ENOTSUP, "'f32'", "'dec'")
    refused([("count", "d")], _ffi.MI_ENOTSUP, "'d'", "COUNT", "dictionary")
    refused([("count", "filename")], _ffi.MI_ENOTSUP, "'filename'", "COUNT", "constant", filename=True)
    refused([("sum", "nope")], _ffi.MI_EINVAL, "'nope'", "SUM")
    refused([("count_star",)] * 9, _ffi.MI_EINVAL, "1 to 8")
    # nine aggregates through the C ABI itself
    rel = con.read_arrow(fx.path, accept_dictionaries=True)
    spec = (_ffi.AggSpec * 9)()
    for s in spec:
        s.op = _ffi.AGG_COUNT_STAR
    out = (_ffi.AggValue * 9)()
    assert _ffi.lib().mi_scan_aggregate(rel._h, spec, 9, out, None, None) == _ffi.MI_EINVAL
    rel.close()
    # after init
    rel = con.read_arrow(fx.path, accept_dictionaries=True).project(["k"])
    assert rel.count() == N
    try:
        with pytest.raises(da.MiError) as e:
            rel.aggregate([("count_star",)])
    finally:
        rel.close()
    assert e.value.code == _ffi.MI_EINVAL and "right after bind" in str(e.value)


def test_an_aggregate_column_absent_from_a_file_is_refused(con, fx, tmp_path):
    other = str(tmp_path / "other.arrows")
    t = pa.table({"k": pa.array(np.arange(10, dtype=np.int64))})
    with ipc.new_stream(other, t.schema) as w:
        w.write_table(t)
    rel = con.read_arrow([fx.path, other], union_by_name=True, accept_dictionaries=True)
    try:
        with pytest.raises(da.MiError) as e:
            rel.aggregate([("sum", "i32")])
    finally:
        rel.close()
    assert e.value.code == _ffi.MI_EINVAL and "'i32'" in str(e.value) and "absent" in str(e.value)
    assert con.read_arrow([fx.path, other], union_by_name=True, accept_dictionaries=True).aggregate([("count_star",), ("max", "k")]) == [N + 10, N - 1]


def test_sum_product_is_still_refused_once_a_filter_was_set(con, fx):
    rel = con.read_arrow(fx.path, accept_dictionaries=True).filter(("i32", ">", 0))
    try:
        with pytest.raises(da.MiError) as e:
            rel.sum_product("i64", "i32")
    finally:
        rel.close()
    assert e.value.code == _ffi.MI_EINVAL and "give the filters to mi_scan_sum_product instead of mi_scan_set_filter" in str(e.value)


def test_plain_c_client_computes_q6_and_its_neighbours(tmp_path):
    """examples/agg.c: the predicates through mi_scan_set_filter, five aggregates through mi_scan_aggregate, from C99"""
    import subprocess
    from test_aggregate_host import build_agg_example
    exe = build_agg_example(tmp_path)
    path = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "lineitem_sf0_01_q6.arrows")
    r = subprocess.run([exe, path], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    py = _read_back(path)
    rows = [i for i in range(len(py["l_shipdate"])) if 8766 <= py["l_shipdate"][i] < 9131 and 5 <= py["l_discount"][i] <= 7 and py["l_quantity"][i] < 2400]
    qty = sum(py["l_quantity"][i] for i in rows)
    assert "revenue = 1193053.2253  (1191 of 60175 rows pass)" in r.stdout and "count(*) = 1191\n" in r.stdout
    assert "l_shipdate in [%d, %d] days" % (min(py["l_shipdate"][i] for i in rows), max(py["l_shipdate"][i] for i in rows)) in r.stdout
    assert "sum(l_quantity) = %d.%02d over 1191 rows" % (qty // 100, qty % 100) in r.stdout
