"""tests/agg_type_cases.py held to what it does not compute itself, without a GPU: (a) the stored values it writes down equal
tests/golden/make_golden.py::canon_column of the Arrow arrays it builds from them, (b) its reference equals pyarrow's sum,
min_max and Table.group_by where pyarrow has the kernel, (c) the decode kinds the host reader binds for the matrix cover every
kind the aggregates read integers through, and (d) every entry declares what each of the three entry points does with it."""
import decimal
import math
import os
import sys

import numpy as np
import pyarrow as pa
import pyarrow.compute as pc
import pytest

import duckdb_arrow_amd as da
from duckdb_arrow_amd import _ffi

import agg_type_cases as tc
import extension_cases as ec

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden"))
from make_golden import canon_column, canon_value  # noqa: E402

# the matrix the issue asks for, by name: an entry that is dropped, or skipped somewhere, shows here
NAMES = ["i8", "i16", "u16", "i32", "i64", "u64", "date32", "date64", "time32_s", "time32_ms", "time64_us", "time64_ns",
         "ts_s", "ts_s_utc", "ts_ms", "ts_ms_utc", "ts_us", "ts_us_utc", "ts_ns", "ts_ns_utc",
         "dec128_1", "dec128_4", "dec128_5", "dec128_9", "dec128_10", "dec128_18", "dec128_19", "dec128_38",
         "dec32_4", "dec32_9", "dec64_4", "dec64_9", "dec64_18", "dec256_40", "f16", "f32", "f64", "bool", "bool8", "uuid",
         "str", "large_string", "string_view", "large_binary", "fsb3", "fsb12", "fsb13", "dur_s", "dur_ms", "dur_us", "dur_ns", "interval",
         "ree_i16", "ree_dec128_9", "ree_ts_ns", "ree_f16", "ree_bool8", "ree_uuid", "ree_str"]


def test_the_matrix_is_whole_and_every_entry_declares_every_entry_point():
    assert [e.name for e in tc.MATRIX] == NAMES and len(NAMES) == 59
    for e in tc.MATRIX:
        assert set(e.expect) == set(tc.ENTRY_POINTS), e.name
        for point, x in e.expect.items():
            assert isinstance(x, (tc.Takes, tc.Refuses)), (e.name, point)
            if not x.takes:
                assert "'%s'" % e.name in x.words and "(%s)" % e.duck in x.words, (e.name, point, x)   # the column and its DuckDB type
        assert len(e.stored) == tc.N
        if e.expect["group_key"].takes:
            assert e.low is not None and len(e.low.stored) == tc.N, e.name
    took = {p: sum(e.expect[p].takes for e in tc.MATRIX) for p in tc.ENTRY_POINTS}
    assert took == {"aggregate": 42, "group_key": 49, "hash_key": 37}, took


@pytest.mark.parametrize("name", NAMES)
def test_nulls_and_edge_rows(name):
    e = tc.BY_NAME[name]
    nulls = sum(v is None for v in e.stored)
    if e.is_ree:
        assert 0 < nulls < tc.N // 3
    else:
        assert 0.10 * tc.N <= nulls <= 0.20 * tc.N, (name, nulls)
        assert all(v is not None for v in e.stored[1:tc.EDGE_ROWS:2])
    assert sum(len(c) for c in e.chunks()) == tc.N and [len(c) for c in e.chunks()] == list(tc.BATCHES)
    assert all(c.type == e.type for c in e.chunks())


def _expanded(chunks):
    """run-end arrays -> their flat values, by the run ends the arrays hold"""
    out = []
    for c in chunks:
        if isinstance(c.type, pa.RunEndEncodedType):
            ends = np.array(c.run_ends.to_pylist(), np.int64)
            assert c.offset == 0 and ends[-1] == len(c)
            c = c.values.take(pa.array(np.searchsorted(ends, np.arange(len(c)), side="right")))
        if isinstance(c.type, pa.BaseExtensionType):
            c = c.storage
        out.append(c)
    return pa.chunked_array(out)


def _same(a, b):
    return a == b or (isinstance(a, float) and isinstance(b, float) and math.isnan(a) and math.isnan(b))


@pytest.mark.parametrize("name", NAMES)
def test_stored_values_equal_canon_column_of_the_built_array(name):
    e = tc.BY_NAME[name]
    for entry in [e] + ([e.low] if e.low is not None and e.low is not e else []):
        for c in entry.chunks():
            c.validate(full=True)
        with decimal.localcontext() as ctx:
            ctx.prec = 80                 # (canon_column scales DECIMALs in the current context: 38 and 40 digits must not round)
            got = canon_column(_expanded(entry.chunks()))
        want = [canon_value(v) for v in entry.canon]
        assert len(got) == len(want) == tc.N
        bad = [r for r in range(tc.N) if not _same(got[r], want[r])]
        assert not bad, (entry.name, bad[:5], [got[r] for r in bad[:5]], [want[r] for r in bad[:5]])
        if entry.type == pa.float16():      # the half a stored float narrows to is the half in the file
            back = np.array([0.0 if v is None else v for v in entry.stored]).astype(np.float16)
            raw = np.frombuffer(entry.array.buffers()[1], np.float16)
            ok = np.array([v is not None for v in entry.stored])
            assert np.array_equal(back[ok].view(np.uint16) & 0x7C00, raw[ok].view(np.uint16) & 0x7C00) and np.array_equal(back[ok], raw[ok], equal_nan=True)


def test_twins_without_nulls_are_their_entries_without_a_bitmap():
    bound = _bound()
    for e, base in zip(tc.TWINS, ("dec64_18", "dec128_4")):
        assert e.name == base + "_nn" and e.name not in NAMES and None not in e.stored and len(set(e.stored)) <= 45
        assert e.array.null_count == 0 and e.array.buffers()[0] is None and e.type == tc.BY_NAME[base].type
        e.array.validate(full=True)
        assert canon_column(pa.chunked_array(e.chunks())) == e.stored
        assert bound[e.name] == bound[base]
    assert bound["dec64_18_nn"][:3] == (_ffi.K_COPY, 8, 8) and bound["dec128_4_nn"][:3] == (_ffi.K_DEC128, 2, 2)
    # the float entries are finite behind row 800, where the third K9 run of the float class looks
    for name in ("f16", "f32", "f64", "ree_f16"):
        assert all(v is None or math.isfinite(v) for v in tc.BY_NAME[name].stored[tc.FINITE_ROWS[0]:]), name
    assert not all(v is None or math.isfinite(v) for v in tc.BY_NAME["ree_f16"].stored[:800])


def test_extension_entries_follow_the_restatement_of_extension_cases():
    e = tc.BY_NAME["bool8"]
    storage = np.array([0 if v is None else v for v in e.canon], np.int8)
    assert [None if c is None else int(b) for c, b in zip(e.canon, ec.bool8(storage))] == e.stored
    assert [e.canon[r] for r in (1, 3, 5, 7)] == [0, 1, 2, -1] and [e.stored[r] for r in (1, 3, 5, 7)] == [0, 1, 1, 1]
    u = tc.BY_NAME["uuid"]
    raw = np.frombuffer(b"".join(bytes(16) if c is None else c for c in u.canon), np.uint8).reshape(-1, 16)
    assert [None if c is None else s for c, s in zip(u.canon, ec.hugeint_of(ec.uuid_from_arrow(raw)))] == u.stored
    assert [u.canon[2 * i + 1] for i in range(len(ec.UUID_EDGES))] == ec.UUID_EDGES
    # the order of the stored integers is the order of the text, which is what MIN / MAX and the key order rely on
    live = [(s, c) for s, c in zip(u.stored, u.canon) if s is not None]
    assert [c for _, c in sorted(live)] == sorted(c for _, c in live)
    assert all(da.uuid_to_hugeint(u.key_out(s)) == s for s, _ in live[:50])


def test_edge_values_the_issue_names():
    s = lambda name: [tc.BY_NAME[name].stored[r] for r in range(1, tc.EDGE_ROWS, 2)]
    assert s("ts_s_utc")[:2] == [9223372036854 * 10 ** 6, -9223372036854 * 10 ** 6] and s("ts_s")[:2] == [9223372036854, -9223372036854]
    assert s("ts_ms_utc")[:2] == [9223372036854775000, -9223372036854775000]
    assert s("ts_us")[:2] == [tc.I64_MIN + 1, tc.I64_MAX] == s("ts_us_utc")[:2]
    assert s("ts_ns")[:6] == [tc.I64_MIN, tc.I64_MAX, -1, -999, -1000, -1001] and s("ts_ns_utc")[:6] == [-9223372036854775, 9223372036854775, 0, 0, -1, -1]
    assert s("time32_s")[0] == 86399 * 10 ** 6 and s("time32_ms")[0] == 86399999000 and s("time64_us")[0] == 86399999999 == s("time64_ns")[0]
    ns = np.frombuffer(tc.BY_NAME["time64_ns"].array.buffers()[1], np.int64)
    assert ns[1] == 86399999999999 and (ns % 1000 != 0).sum() > tc.N // 2
    assert min(v for v in tc.BY_NAME["date64"].stored if v is not None) == -(1 << 31)
    for name, p in (("dec128_1", 1), ("dec128_4", 4), ("dec128_5", 5), ("dec128_9", 9), ("dec128_10", 10), ("dec128_18", 18), ("dec128_19", 19), ("dec128_38", 38),
                    ("dec32_4", 4), ("dec32_9", 9), ("dec64_4", 4), ("dec64_9", 9), ("dec64_18", 18), ("dec256_40", 40)):
        assert s(name)[:4] == [10 ** p - 1, -(10 ** p - 1), 0, -1], name
    f = s("f16")
    assert f[:6] == [65504.0, -65504.0, 2.0 ** -24, -(2.0 ** -24), 0.0, 0.0] and math.copysign(1, f[5]) == -1 and f[6:8] == [math.inf, -math.inf]
    assert math.isnan(f[8]) and math.isnan(f[9])
    halves = np.frombuffer(tc.BY_NAME["f16"].array.buffers()[1], np.uint16)
    assert halves[17] >> 15 == 0 and halves[19] >> 15 == 1          # NaNs of both signs in the file
    assert {len(v) for v in tc.BY_NAME["fsb13"].stored if v is not None} == {13} and tc.BY_NAME["fsb13"].long_key


# ------------------------------------------------------------------------------------------------ (b) the reference
def _int64_entries():
    return [e for e in tc.MATRIX if e.cls in (tc.INT, tc.UINT) and all(v is None or tc.I64_MIN <= v <= tc.I64_MAX for v in e.stored)]


def test_wrap128_is_the_scan_tests_wrap():
    from test_gpu_scan_aggregate import _wrap128
    for v in (0, -1, 1 << 127, (1 << 127) - 1, -(1 << 127), -(1 << 127) - 1, 3 << 130, -(5 << 129) + 7):
        assert tc.wrap128(v) == _wrap128(v)


@pytest.mark.parametrize("name", [e.name for e in _int64_entries()])
def test_reference_against_pyarrow_on_the_stored_integers(name):
    e = tc.BY_NAME[name]
    stored = dict(v=e.stored, g=tc.companions()["g"][0], k=list(range(tc.N)))
    arr = pa.array(e.stored, pa.int64())
    fits = sum(abs(v) for v in e.stored if v is not None) < 1 << 63
    for rows in (list(range(tc.N)), tc.FILTER_ROWS):
        part = arr.take(pa.array(rows))
        mm = pc.min_max(part).as_py()
        assert tc.expected(("min", "v"), stored, rows) == ("exact", mm["min"]) and tc.expected(("max", "v"), stored, rows) == ("exact", mm["max"])
        assert tc.expected(("count", "v"), stored, rows) == ("exact", pc.count(part).as_py())
        if fits:
            assert tc.expected(("sum", "v"), stored, rows) == ("exact", pc.sum(part).as_py())
    specs = [("count_star",), ("count", "v"), ("min", "v"), ("max", "v")] + ([("sum", "v")] if fits else [])
    t = pa.table({"g": pa.array(stored["g"], pa.int16()), "v": arr})
    pa_groups = t.group_by("g").aggregate([([], "count_all"), ("v", "count"), ("v", "min"), ("v", "max"), ("v", "sum")]).to_pylist()
    want = {r["g"]: [r["count_all"], r["v_count"], r["v_min"], r["v_max"]] + ([r["v_sum"]] if fits else []) for r in pa_groups}
    got = tc.expected_groups("g", specs, stored, range(tc.N))
    assert [k for k, _ in got] == sorted(want, key=tc.order_key) and len(got) == 41
    for k, values in got:
        assert [v for _, v in values] == want[k], (k, values, want[k])


@pytest.mark.parametrize("name", ["dec128_1", "dec128_4", "dec128_9", "dec128_18", "dec128_19", "dec128_38", "dec32_9", "dec64_18"])
def test_reference_against_pyarrow_decimal_kernels(name):
    e = tc.BY_NAME[name]
    stored = dict(v=e.stored)
    with decimal.localcontext() as ctx:
        ctx.prec = 80
        unscaled = lambda d: int(d.scaleb(e.type.scale))
        arr = e.array if e.type.bit_width == 128 else e.array.cast(pa.decimal128(e.type.precision, e.type.scale))
        for rows in (list(range(tc.N)), tc.FILTER_ROWS):
            part = arr.take(pa.array(rows))
            mm = pc.min_max(part).as_py()
            assert tc.expected(("min", "v"), stored, rows) == ("exact", unscaled(mm["min"])) and tc.expected(("max", "v"), stored, rows) == ("exact", unscaled(mm["max"]))
            if e.type.precision <= 18:
                assert tc.expected(("sum", "v"), stored, rows) == ("exact", unscaled(pc.sum(part).as_py()))


@pytest.mark.parametrize("name", ["f32", "f64", "f16"])
def test_float_reference_against_pyarrow_and_numpy(name):
    e = tc.BY_NAME[name]
    stored = dict(v=e.stored)
    rows = tc.FILTER_ROWS
    live = [e.stored[r] for r in rows if e.stored[r] is not None]
    kind, terms = tc.expected(("sum", "v"), stored, rows)
    assert kind == "sum" and len(terms) == len(live)
    with np.errstate(invalid="ignore"):
        tc.check(float(np.sum(np.array(live, np.float64))), (kind, terms), name)   # numpy's pairwise sum is one of the orders
    if name != "f16":
        mm = pc.min_max(pa.array(live, pa.float64())).as_py()
        for op in ("min", "max"):
            tc.check(mm[op] + 0.0, tc.expected((op, "v"), stored, rows), (name, op))
    else:               # NaN is the greatest value, -inf the least
        assert math.isnan(tc.expected(("max", "v"), stored, rows)[1]) and tc.expected(("min", "v"), stored, rows)[1] == -math.inf
        with pytest.raises(AssertionError):
            tc.check(1.0, (kind, terms), "a finite sum where NaN is due")
    finite = [t for t in terms if math.isfinite(t)]
    bound = 2 * len(finite) * 2.0 ** -53 * math.fsum(abs(t) for t in finite)
    tc.check(math.fsum(finite) + 0.5 * bound, ("sum", finite), "inside the bound")
    with pytest.raises(AssertionError):
        tc.check(math.fsum(finite) + 2 * bound, ("sum", finite), "outside the bound")


def test_sum_expr_and_sum_product_terms():
    stored = dict(a=[2, None, -3], b=[5, 7, None], f=[0.5, None, -1.25])
    assert tc.expected(("sum_product", "a", "b"), stored, range(3)) == ("exact", 10)
    assert tc.expected(("sum_expr", ("a", 3, -7), 5), stored, range(3)) == ("exact", (-7 + 6) * 5 + (-7 - 9) * 5)
    assert tc.expected(("sum_expr", ("f", 4.0, 0.0), 0.5), stored, range(3)) == ("sum", [1.0, -2.5])
    assert tc.expected(("sum", "a"), stored, [1]) == ("exact", None) and tc.expected(("count", "a"), stored, [1]) == ("exact", 0)
    big = dict(a=[(1 << 127) - 1, 1])
    assert tc.expected(("sum", "a"), big, range(2)) == ("exact", -(1 << 127))


# ------------------------------------------------------------------------------------------------ (c) the decode kinds
def _bound():
    """{column: (kind, param, out_width)} as the host reader binds the two files"""
    files, _ = tc.tables()
    out = {}
    for schema, batches in files.values():
        r = da.Reader(buffers=[ec.ipc_stream(batches, schema)])
        try:
            out.update({f["name"]: (f["kind"], f["param"], f["out_width"], f["duck_type"]) for f in r.schema()})
        finally:
            r.close()
    return out


def test_the_matrix_covers_every_decode_kind_the_aggregates_read():
    bound = _bound()
    for e in tc.MATRIX:
        assert bound[e.name][3] == e.duck, (e.name, bound[e.name])
    plans = {bound[e.name][:3] for e in tc.MATRIX}
    flat = {(k, p, w) for k, p, w in plans if k != _ffi.K_RUN_END}
    # every (kind, param, out_width) ArrowField::Plan produces for which IsIntegerLike holds, as literals
    integer_like = {(_ffi.K_COPY, 1, 1), (_ffi.K_COPY, 2, 2), (_ffi.K_COPY, 4, 4), (_ffi.K_COPY, 8, 8),
                    (_ffi.K_DEC128, 2, 2), (_ffi.K_DEC128, 4, 4), (_ffi.K_DEC128, 8, 8),
                    (_ffi.K_NARROW, 4 | (2 << 8), 2), (_ffi.K_NARROW, 8 | (2 << 8), 2), (_ffi.K_NARROW, 8 | (4 << 8), 4),
                    (_ffi.K_DATE64, 0, 4), (_ffi.K_MUL_I32, 1000000, 8), (_ffi.K_MUL_I32, 1000, 8),
                    (_ffi.K_MUL_I64, 1000000, 8), (_ffi.K_MUL_I64, 1000, 8), (_ffi.K_DIV_I64, 1000, 8)}
    others = {(_ffi.K_COPY, 16, 16), (_ffi.K_UUID, 16, 16), (_ffi.K_BOOL, 0, 1), (_ffi.K_BOOL8, 1, 1), (_ffi.K_HALF_FLOAT, 0, 4),
              (_ffi.K_STR32, 0, 16), (_ffi.K_STR64, 0, 16), (_ffi.K_STRVIEW, 0, 16), (_ffi.K_FIXED_BINARY, 3, 16), (_ffi.K_FIXED_BINARY, 12, 16),
              (_ffi.K_FIXED_BINARY, 13, 16), (_ffi.K_DURATION, 1000000, 16), (_ffi.K_DURATION, 1000, 16), (_ffi.K_DURATION, 1, 16),
              (_ffi.K_DURATION, -1000, 16), (_ffi.K_INTERVAL_MDN, 0, 16), (0, 0, 0)}     # (0, 0, 0): decimal256, which has no plan
    assert flat == integer_like | others, (sorted(flat - integer_like - others), sorted((integer_like | others) - flat))
    # the two float classes are COPY 4 / COPY 8 of a FLOAT / DOUBLE column
    assert bound["f32"][:3] == (_ffi.K_COPY, 4, 4) and bound["f64"][:3] == (_ffi.K_COPY, 8, 8)
    # which entry binds to which kind: the representatives the scan-mode tests pick rely on this
    want = dict(dec128_4=(_ffi.K_DEC128, 2, 2), dec128_5=(_ffi.K_DEC128, 4, 4), dec128_9=(_ffi.K_DEC128, 4, 4), dec128_10=(_ffi.K_DEC128, 8, 8),
                dec32_4=(_ffi.K_NARROW, 4 | (2 << 8), 2), dec64_4=(_ffi.K_NARROW, 8 | (2 << 8), 2), dec64_9=(_ffi.K_NARROW, 8 | (4 << 8), 4),
                dec32_9=(_ffi.K_COPY, 4, 4), dec64_18=(_ffi.K_COPY, 8, 8), date64=(_ffi.K_DATE64, 0, 4), time32_s=(_ffi.K_MUL_I32, 1000000, 8),
                time64_ns=(_ffi.K_DIV_I64, 1000, 8), ts_s_utc=(_ffi.K_MUL_I64, 1000000, 8), ts_ms_utc=(_ffi.K_MUL_I64, 1000, 8),
                ts_ns_utc=(_ffi.K_DIV_I64, 1000, 8), ts_s=(_ffi.K_COPY, 8, 8), ts_ns=(_ffi.K_COPY, 8, 8), dec128_19=(_ffi.K_COPY, 16, 16))
    assert {k: bound[k][:3] for k in want} == want
    # run ends of 2, 4 and 8 bytes over values of 1, 2, 4, 8 and 16 bytes: param = run-end bytes | value width << 8
    ree = {bound[e.name][:3] for e in tc.MATRIX if e.is_ree}
    assert ree == {(_ffi.K_RUN_END, 2 | (2 << 8), 2), (_ffi.K_RUN_END, 4 | (4 << 8), 4), (_ffi.K_RUN_END, 8 | (8 << 8), 8), (_ffi.K_RUN_END, 2 | (4 << 8), 4),
                   (_ffi.K_RUN_END, 4 | (1 << 8), 1), (_ffi.K_RUN_END, 8 | (16 << 8), 16), (_ffi.K_RUN_END, 2 | (16 << 8), 16)}
    assert len({w for _, _, w in ree}) >= 3
    # the low-cardinality key variants bind as their entries do
    for e in tc.MATRIX:
        if e.low is not None and e.low is not e:
            assert bound[e.low.name] == bound[e.name], e.name


def test_low_cardinality_variants_keep_the_edges_and_fit_a_window():
    for e in tc.MATRIX:
        if not e.expect["group_key"].takes:
            continue
        low = e.low
        for first in range(0, tc.N, tc.W):
            assert len({repr(v) for v in low.stored[first: first + tc.W]}) <= 200, (e.name, first)
        if low is not e:
            assert low.stored[1:tc.EDGE_ROWS:2] == e.stored[1:tc.EDGE_ROWS:2], e.name
            assert low.type == e.type and low.cls == e.cls and low.duck == e.duck
