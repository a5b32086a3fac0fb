"""MI_AGG_SUM_EXPR through the scan (mi_scan_aggregate, mi_scan_group_aggregate): TPC-H Q1 whole as ONE group_aggregate call
on the golden lineitem, and expression sums under every filter form, consumer, body compression and sharding, against
tests/agg_expr_cases.py (Python ints modulo 2^128, Fractions) over pyarrow's reading of the same file.  Expected values
never come from the library.  Integer results are exact; double results within 2 (n + 3 F) 2^-53 sum|term| (agg_expr_cases.py)."""
import datetime
import decimal
import os
import subprocess

import numpy as np
import pyarrow as pa
import pyarrow.compute as pc
import pyarrow.ipc as ipc
import pytest

import duckdb_arrow_amd as da
from duckdb_arrow_amd import _ffi

import agg_expr_cases as ec

pytestmark = pytest.mark.gpu

HERE = os.path.dirname(os.path.abspath(__file__))
LINEITEM = os.path.join(HERE, "golden", "lineitem_sf0_01_head.arrows")
N = 9000
BATCH_ROWS = 2500      # four record batches: more than the pipeline's slots, a ragged last window in each
CTX = decimal.Context(prec=60)
EPOCH = datetime.date(1970, 1, 1)
I64_MIN = ec.I64_MIN
MODES = [dict(device_resident=True), dict(), dict(device_resident=True, unset_all_valid=True, zero_copy_direct=True),
         dict(unset_all_valid=True, zero_copy_direct=False)]
WORDS = ["special", "regular", "express", "pending", "final", "ironic", "bold", "quick packages", "carefully special requests", ""]
MODES_OF_SHIP = ["MAIL", "SHIP", "RAIL", "AIR", "TRUCK", "REG AIR", "FOB"]


@pytest.fixture(scope="module")
def con():
    return da.Connection(0)


def _stored(v, t):
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
            out[name] = [_stored(v, t.value_type) for chunk in col.chunks for v in pc.run_end_decode(chunk).to_pylist()]
            continue
        if t == pa.float16():
            out[name] = [None if v is None else float(v) for v in col.to_pylist()]
            continue
        out[name] = [_stored(v, t) for v in col.to_pylist()]
    return out


class Fixture:
    pass


def _table():
    rng = np.random.default_rng(777)
    mask = lambda: rng.random(N) < rng.uniform(0.10, 0.20)
    arrays = {"k": pa.array(np.arange(N, dtype=np.int64))}
    for name, t in (("i8", np.int8), ("i16", np.int16), ("i32", np.int32), ("i64", np.int64), ("u8", np.uint8), ("u16", np.uint16),
                    ("u32", np.uint32), ("u64", np.uint64)):
        info = np.iinfo(t)
        v = rng.integers(info.min, info.max, N, dtype=t, endpoint=True)
        v[:3] = [info.min, info.max, info.max]
        arrays[name] = pa.array(v, mask=mask())
    arrays["n64"] = pa.array(rng.integers(-10 ** 6, 10 ** 6, N).astype(np.int64))          # no NULL: zero_copy_direct aliases it
    arrays["f32"] = pa.array(rng.normal(0, 100, N).astype(np.float32), mask=mask())
    arrays["f64"] = pa.array(rng.normal(0, 1e4, N) * rng.choice([1e-6, 1.0, 1e6], N), mask=mask())
    arrays["f16"] = pa.array((np.round(rng.normal(0, 40, N)) / 4).astype(np.float16), mask=mask())
    arrays["g64"] = pa.array(rng.normal(1, 0.5, N))                                         # no NULL
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
    arrays["b"] = pa.array(rng.random(N) < 0.5, mask=mask())
    m = mask()
    arrays["lst"] = pa.array([None if x else list(range(i % 4)) for i, x in enumerate(m)], pa.list_(pa.int32()))
    arrays["iv"] = pa.array([pa.MonthDayNano([1, 2, 3])] * N, pa.month_day_nano_interval())
    arrays["grp"] = pa.array(rng.integers(0, 5, N).astype(np.int8), mask=mask())
    return pa.table(arrays)


def _write(path, table, **options):
    with ipc.new_stream(path, table.schema, options=ipc.IpcWriteOptions(**options) if options else None) as w:
        w.write_table(table, max_chunksize=BATCH_ROWS)


@pytest.fixture(scope="module")
def fx(tmp_path_factory):
    f = Fixture()
    d = tmp_path_factory.mktemp("agg_expr")
    f.table = _table()
    f.path = str(d / "t.arrows")
    _write(f.path, f.table)
    assert [b.num_rows for b in ipc.open_stream(f.path)] == [2500, 2500, 2500, 1500]
    f.lz4, f.zstd = str(d / "lz4.arrows"), str(d / "zstd.arrows")
    _write(f.lz4, f.table, compression="lz4")
    _write(f.zstd, f.table, compression="zstd")
    f.dict = str(d / "dict.arrows")
    _write(f.dict, pa.table({"k": f.table.column("k"), "i32": f.table.column("i32"), "d": f.table.column("s").combine_chunks().dictionary_encode()}))
    f.py = _read_back(f.path)
    return f


EXPRS = [("sum_expr", "dec", ("i8", -1, 100), ("u16", 1, 100)),                 # Q1's sum_charge shape over mixed widths
         ("sum_expr", "i64", "i32"),
         ("sum_expr", ("date", 1, -8000), ("u8", 0, 3), "i16", 7),              # four factors, a mul of 0, a constant
         ("sum_expr", "u64", "u64", ("i64", -1, I64_MIN)),                      # wraps modulo 2^128
         ("sum_expr", "n64", "n64"),                                            # a column without NULLs, twice
         ("sum_expr", "f64", ("f32", -1.0, 1.0)),
         ("sum_expr", "f16", "g64", ("f64", 0.5, 2.0)),
         ("sum_expr", ("g64", 3, -1))]


def factors_of(py, spec):
    out = []
    for f in spec[1:]:
        if isinstance(f, str):
            f = (f, 1, 0)
        if isinstance(f, tuple):
            col = py[f[0]]
            out.append(ec.Factor([0 if v is None else v for v in col], [v is not None for v in col], f[1], f[2]))
        else:
            out.append(ec.Factor(None, None, 1, f))
    return out


def is_float_expr(py, spec):
    return any(isinstance(v, float) for f in spec[1:] if isinstance(f, (str, tuple)) for v in py[f if isinstance(f, str) else f[0]][:50] if v is not None)


def check_expr(py, spec, rows, got, what):
    """got: (value, count)"""
    factors = factors_of(py, spec)
    if is_float_expr(py, spec):
        ec.check_float(got, factors, rows, str(what))
    else:
        assert got == ec.sum_expr_int(factors, rows), (what, spec, got)


def _like(parts):
    def match(v):
        at = 0
        for p in parts:
            at = v.find(p, at)
            if at < 0:
                return False
            at += len(p)
        return True
    return match


FILTERS = {
    "none": (None, lambda py, r: True),
    "range": (("and", ("i32", ">=", -(1 << 30)), ("i32", "<", 1 << 30)), lambda py, r: py["i32"][r] is not None and -(1 << 30) <= py["i32"][r] < (1 << 30)),
    "in": (("i8", "in", list(range(-40, 40, 3))), lambda py, r: py["i8"][r] in set(range(-40, 40, 3))),
    "string": (("s", "in", ["MAIL", "SHIP"]), lambda py, r: py["s"][r] in ("MAIL", "SHIP")),
    "like": (("c", "like", "%special%req%"), lambda py, r: py["c"][r] is not None and _like(["special", "req"])(py["c"][r])),
    "float": (("f32", ">", 12.5), lambda py, r: py["f32"][r] is not None and py["f32"][r] > 12.5),
    "or-tree": (("or", ("i16", "<", -20000), ("f64", ">", 1e3)),
                lambda py, r: (py["i16"][r] is not None and py["i16"][r] < -20000) or (py["f64"][r] is not None and py["f64"][r] > 1e3)),
}


def _values_with_counts(rel, specs):
    """the contributing rows of an ungrouped aggregate come back through the C struct's `count`: ask the library directly"""
    checked = da._agg_check_specs(specs)
    arr, keep = da._agg_scan_specs(checked)
    out = (_ffi.AggValue * len(checked))()
    import ctypes as C
    scanned, selected = C.c_int64(), C.c_int64()
    _ffi.check(_ffi.lib().mi_scan_aggregate(rel._h, arr, len(checked), out, C.byref(scanned), C.byref(selected)))
    rel._initialised = True
    return [(da._agg_value(v), v.count) for v in out], scanned.value, selected.value


@pytest.mark.parametrize("name", list(FILTERS))
def test_expression_sums_under_every_filter_form_and_consumer(con, fx, name):
    expr, keep = FILTERS[name]
    rows = [r for r in range(N) if keep(fx.py, r)]
    assert 0 < len(rows) <= N and (expr is None or len(rows) < N)
    for mode in MODES:      # device-resident (zero_copy_direct: n64 and g64 are aliases of the body) and host consumers
        rel = con.read_arrow(fx.path, **mode)
        rel = rel.filter(expr) if expr is not None else rel
        got, scanned, selected = _values_with_counts(rel, EXPRS)
        assert (scanned, selected) == (N, len(rows)), (name, mode)
        for sp, g in zip(EXPRS, got):
            check_expr(fx.py, sp, rows, g, (name, mode))
        rel = con.read_arrow(fx.path, **mode)
        assert (rel.filter(expr) if expr is not None else rel).aggregate(EXPRS) == [v for v, _ in got]      # the public call, bit for bit again


def test_equivalences_through_the_scan_bit_for_bit(con, fx):
    specs = [("sum_expr", "f64"), ("sum", "f64"), ("sum_expr", "f32", "f64"), ("sum_product", "f32", "f64"), ("sum_expr", "u64", "i8"),
             ("sum_product", "u64", "i8"), ("sum_expr", "dec"), ("sum", "dec")]
    for mode in MODES[:2]:
        for expr in (None, ("c", "like", "%special%")):
            rel = con.read_arrow(fx.path, **mode)
            got = (rel.filter(expr) if expr else rel).aggregate(specs)
            for i in range(0, len(specs), 2):
                a, b = got[i], got[i + 1]
                assert (ec.bits(a) == ec.bits(b)) if isinstance(a, float) else (a == b and isinstance(a, int)), (specs[i], a, b)
            rel = con.read_arrow(fx.path, **mode)
            grouped = (rel.filter(expr) if expr else rel).group_aggregate(["grp"], specs)
            assert len(grouped) == 6
            for key, vals in grouped:
                for i in range(0, len(specs), 2):
                    a, b = vals[i], vals[i + 1]
                    assert (ec.bits(a) == ec.bits(b)) if isinstance(a, float) else a == b, (key, specs[i], a, b)


@pytest.mark.parametrize("codec", ["lz4", "zstd"])
def test_compressed_bodies(con, fx, codec):
    path = getattr(fx, codec)
    rows = [r for r in range(N) if fx.py["k"][r] >= 1234]
    for mode in MODES[:2]:
        rel = con.read_arrow(path, **mode).filter(("k", ">=", 1234))
        got, scanned, selected = _values_with_counts(rel, EXPRS)
        assert (scanned, selected) == (N, len(rows))
        for sp, g in zip(EXPRS, got):
            check_expr(fx.py, sp, rows, g, (codec, mode))
    # and with the bodies decompressed in HBM (K8), whichever codec the default would leave to the host
    rel = con.read_arrow(path, device_resident=True, host_decompress="gpu").filter(("k", ">=", 1234))
    got, scanned, selected = _values_with_counts(rel, EXPRS)
    for sp, g in zip(EXPRS, got):
        check_expr(fx.py, sp, rows, g, (codec, "decompressed on the device"))
    assert rel.stats()["lz4_batches_on_device" if codec == "lz4" else "zstd_batches_on_device"] == 4


def test_run_end_encoded_factor_column(con, tmp_path):
    rng = np.random.default_rng(8)
    n, per_batch = 9000, 4500
    path = str(tmp_path / "ree.arrows")
    schema = pa.schema([("r", pa.run_end_encoded(pa.int32(), pa.int64())), ("k", pa.int64()), ("w", pa.int16())])
    with ipc.new_stream(path, schema) as w:
        for first in range(0, n, per_batch):
            ends = np.cumsum(rng.integers(1, 40, 400))
            ends = ends[ends < per_batch].tolist() + [per_batch]
            values = [None if rng.random() < 0.15 else int(v) for v in rng.integers(-10 ** 12, 10 ** 12, len(ends))]
            ree = pa.RunEndEncodedArray.from_arrays(pa.array(ends, pa.int32()), pa.array(values, pa.int64()))
            w.write_batch(pa.record_batch([ree, pa.array(np.arange(first, first + per_batch, dtype=np.int64)),
                                           pa.array(rng.integers(-300, 300, per_batch).astype(np.int16), mask=rng.random(per_batch) < 0.1)], schema=schema))
    py = _read_back(path)
    assert any(v is None for v in py["r"])
    specs = [("sum_expr", "r", ("w", -1, 100)), ("sum_expr", ("r", 3, 1), "r"), ("sum_expr", "w", ("r", 0, I64_MIN))]
    for expr, rows in ((None, list(range(n))), (("k", ">=", 2500), list(range(2500, n)))):
        for mode in MODES:
            rel = con.read_arrow(path, **mode)
            got, _, selected = _values_with_counts(rel.filter(expr) if expr else rel, specs)
            assert selected == len(rows)
            for sp, g in zip(specs, got):
                check_expr(py, sp, rows, g, ("ree", expr, mode))


def test_two_contexts_and_rank_world_shares_add_up(con, fx):
    expr = ("c", "like", "%special%")
    rows = [r for r in range(N) if fx.py["c"][r] is not None and "special" in fx.py["c"][r]]
    runs = []
    for _ in range(2):
        rel = con.read_arrow(fx.path, contexts=[da.Context(0), da.Context(0)], device_resident=True).filter(expr)
        got, scanned, selected = _values_with_counts(rel, EXPRS)
        assert (scanned, selected) == (N, len(rows))
        for sp, g in zip(EXPRS, got):
            check_expr(fx.py, sp, rows, g, "two contexts")
        runs.append([(ec.bits(v) if isinstance(v, float) else v, c) for v, c in got])
    assert runs[0] == runs[1]      # the two-context double sums are bit-reproducible
    rel = con.read_arrow(fx.path, contexts=[da.Context(0), da.Context(0)], device_resident=True).filter(expr)
    grouped = rel.group_aggregate(["grp"], EXPRS, detail=True)[0]
    by_key = {}
    for r in rows:
        by_key.setdefault(fx.py["grp"][r], []).append(r)
    assert [k for (k,), _ in grouped] == sorted(k for k in by_key if k is not None) + [None]
    for (k,), vals in grouped:
        for sp, v in zip(EXPRS, vals):
            n = len(ec.contributing(factors_of(fx.py, sp), by_key[k]))
            check_expr(fx.py, sp, by_key[k], (v, n), ("two contexts, grouped", k))
    # rank / world = 2: each rank returns its share, and the shares add up
    parts = [_values_with_counts(con.read_arrow(fx.path, rank=r, world=2).filter(expr), EXPRS) for r in range(2)]
    assert sum(p[1] for p in parts) == N and sum(p[2] for p in parts) == len(rows)
    for i, sp in enumerate(EXPRS):
        (a, ca), (b, cb) = parts[0][0][i], parts[1][0][i]
        factors = factors_of(fx.py, sp)
        if is_float_expr(fx.py, sp):
            exact, total_abs, n = ec.sum_expr_float(factors, rows)
            assert ca + cb == n
            # one more addition than the scan's own fold: n + 1 in place of n in the bound
            assert abs(ec.Fraction(a) + ec.Fraction(b) - exact) <= ec.float_bound(n + 1, len(factors), total_abs), sp
        else:
            assert (ec.wrap128(a + b), ca + cb) == ec.sum_expr_int(factors, rows), sp


def test_q1_whole_as_one_group_aggregate_call(con):
    t = ipc.open_stream(LINEITEM).read_all()
    shipdate = [(d - EPOCH).days for d in t.column("l_shipdate").to_pylist()]
    keys = ["l_returnflag", "l_linestatus"]
    for expr, keep in ((None, lambda r: True), (("l_shipdate", "<=", 10471), lambda r: shipdate[r] <= 10471), (("l_shipdate", "<=", 9500), lambda r: shipdate[r] <= 9500)):
        rows = [r for r in range(t.num_rows) if keep(r)]
        want = ec.q1_reference(t.take(pa.array(rows, pa.int64())))
        assert len(want) >= 3
        for mode in MODES:
            rel = con.read_arrow(LINEITEM, **mode)
            got, scanned, selected = (rel.filter(expr) if expr else rel).group_aggregate(keys, ec.Q1_SPECS, detail=True)
            assert (scanned, selected) == (t.num_rows, len(rows))
            assert [k for k, _ in got] == sorted(want) and [v for _, v in got] == [want[k] for k in sorted(want)], (expr, mode)
    # the averages are the client's division: sum / count
    (key, v) = got[0]
    assert v[5] > 0 and abs(v[0] / 100 / v[5] - 25.5) < 5


def test_plain_c_client_prints_the_whole_of_q1(tmp_path):
    """examples/q1_full.c: six aggregates, two of them expressions, in one mi_scan_group_aggregate call from C99"""
    from test_agg_expr_host import build_q1_full_example
    exe = build_q1_full_example(tmp_path)
    r = subprocess.run([exe, LINEITEM], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    t = ipc.open_stream(LINEITEM).read_all()
    rows = [i for i, d in enumerate(t.column("l_shipdate").to_pylist()) if (d - EPOCH).days <= 10471]
    want = ec.q1_reference(t.take(pa.array(rows, pa.int64())))
    lines = r.stdout.splitlines()
    assert lines[0] == "%d groups, %d of %d rows pass" % (len(want), len(rows), t.num_rows)
    body = lines[2:]
    assert len(want) == 4 and len(body) == 4
    dec = lambda x, unit, digits: "%d.%0*d" % (x // unit, digits, x % unit)
    for line, key in zip(body, sorted(want)):
        v = want[key]
        assert line.split() == [key[0], key[1], dec(v[0], 100, 2), dec(v[1], 100, 2), dec(v[2], 10000, 4), dec(v[3], 1000000, 6),
                                "%.6f" % (v[0] / 100.0 / v[5]), "%.6f" % (v[1] / 100.0 / v[5]), "%.6f" % (v[4] / 100.0 / v[5]), str(v[5])], (line, key, v)


def test_a_factor_column_absent_from_a_file_is_refused(con, fx, tmp_path):
    other = str(tmp_path / "other.arrows")
    t = pa.table({"k": pa.array(np.arange(10, dtype=np.int64)), "i64": pa.array(np.arange(10, dtype=np.int64))})
    with ipc.new_stream(other, t.schema) as w:
        w.write_table(t)
    for call in (lambda rel: rel.aggregate([("sum_expr", "i64", ("i32", -1, 100))]), lambda rel: rel.group_aggregate(["k"], [("sum_expr", "i64", ("i32", -1, 100))])):
        rel = con.read_arrow([fx.path, other], union_by_name=True)
        try:
            with pytest.raises(da.MiError) as e:
                call(rel)
        finally:
            rel.close()
        assert e.value.code == _ffi.MI_EINVAL and "'i32'" in str(e.value) and "absent" in str(e.value)
    rel = con.read_arrow([fx.path, other], union_by_name=True)
    assert rel.aggregate([("count_star",), ("sum_expr", "k", "k")]) == [N + 10, sum(k * k for k in range(N)) + sum(k * k for k in range(10))]


def test_bind_time_refusals_by_code_and_by_column_and_the_relation_still_answers(con, fx):
    def refused(specs, code, *words, path=fx.path, **options):
        for grouped in (False, True):
            rel = con.read_arrow(path, **options)
            try:
                with pytest.raises(da.MiError) as e:
                    rel.group_aggregate(["k"], specs) if grouped else rel.aggregate(specs)
                assert e.value.code == code, (specs, e.value.code, str(e.value))
                for w in words:
                    assert w in str(e.value), (specs, w, str(e.value))
                assert rel.aggregate([("count_star",)]) == [len(ipc.open_stream(path).read_all())]      # the same relation still answers
            finally:
                rel.close()

    refused([("sum_expr", "i32", "f64")], _ffi.MI_ENOTSUP, "'i32'", "'f64'", "both factors must be integer-like or both floating point")
    refused([("sum_expr", "f32", 2, "dec")], _ffi.MI_ENOTSUP, "'f32'", "'dec'")
    refused([("sum_expr", ("i32", 1.5, 0.0))], _ffi.MI_ENOTSUP, "'i32'", "double constants")
    refused([("sum_expr", "i32", 0.5)], _ffi.MI_ENOTSUP, "double constants")
    refused([("sum_expr", "i64", "hug")], _ffi.MI_ENOTSUP, "'hug'", "SUM_EXPR")
    refused([("sum_expr", "b")], _ffi.MI_ENOTSUP, "'b'", "BOOLEAN")
    refused([("sum_expr", "i8", "s")], _ffi.MI_ENOTSUP, "'s'", "VARCHAR")
    refused([("sum_expr", "iv")], _ffi.MI_ENOTSUP, "'iv'")
    refused([("sum_expr", ("lst", 2, 1))], _ffi.MI_ENOTSUP, "'lst'")
    refused([("sum_expr", "i32", "d")], _ffi.MI_ENOTSUP, "'d'", "dictionary", path=fx.dict, accept_dictionaries=True)
    refused([("sum_expr", "i32", "filename")], _ffi.MI_ENOTSUP, "'filename'", "constant", filename=True)
    refused([("sum_expr", "i32", "nope")], _ffi.MI_EINVAL, "'nope'")
    refused([("sum_expr", ("f64", (1 << 53) + 1, 0))], _ffi.MI_EINVAL, "'f64'", "not exactly representable")
    # through the C ABI itself: a NULL expr, F outside 1 .. 4, no factor with a column
    rel = con.read_arrow(fx.path)
    out = (_ffi.AggValue * 1)()
    spec = (_ffi.AggSpec * 1)()
    spec[0].op = _ffi.AGG_SUM_EXPR
    assert _ffi.lib().mi_scan_aggregate(rel._h, spec, 1, out, None, None) == _ffi.MI_EINVAL and "without an expression" in _ffi.lib().mi_last_error().decode()
    e = _ffi.AggExpr()
    import ctypes as C
    spec[0].expr = C.pointer(e)
    for n in (0, 5, -1):
        e.n_factors = n
        assert _ffi.lib().mi_scan_aggregate(rel._h, spec, 1, out, None, None) == _ffi.MI_EINVAL and "1 to 4 factors" in _ffi.lib().mi_last_error().decode()
    e.n_factors = 2
    e.factors[0].add = 3
    e.factors[1].add = 4
    assert _ffi.lib().mi_scan_aggregate(rel._h, spec, 1, out, None, None) == _ffi.MI_EINVAL and "at least one factor with a column" in _ffi.lib().mi_last_error().decode()
    assert rel.aggregate([("count_star",), ("sum_expr", ("k", 0, 4), 3)]) == [N, 12 * N]
    rel.close()
