"""The fused aggregates through the scan over every column type of tests/agg_type_cases.py: mi_scan_aggregate (K9),
mi_scan_group_aggregate (K10) and mi_scan_hash_aggregate (K11) on columns that reach the kernels through every decode kind --
narrowed and copied decimals, date64, time32 / time64, timestamps of every unit with and without a time zone, half floats,
bool8, UUID, the string kinds, and run-end arrays over them -- against the dict loop of the case module over the stored values
it wrote down.  Expected values never come from the library.  Everything is exact but float sums, which are held to
2 n 2^-53 fsum|v| (agg_type_cases.check, the bound of test_gpu_scan_aggregate.py).

One file of 2 * 2048 + 904 rows in record batches of 3000 and 2000 holds the flat entries, a second one the run-end entries."""
import math

import numpy as np
import pyarrow as pa
import pyarrow.ipc as ipc
import pytest

import duckdb_arrow_amd as da
from duckdb_arrow_amd import _ffi

import agg_type_cases as tc
from test_gpu_scan_aggregate import MODES

pytestmark = pytest.mark.gpu

N = tc.N
HASH_GROUPS = 8192
RUNS = [("every row", None, list(range(N))), ("two windows partly selected", tc.FILTER, tc.FILTER_ROWS)]
TAKEN_BY_K9 = [e.name for e in tc.MATRIX if e.expect["aggregate"].takes]
REFUSED_BY_K9 = [e.name for e in tc.MATRIX if not e.expect["aggregate"].takes]
K10_KEYS = [e.name for e in tc.MATRIX if e.expect["group_key"].takes]
K11_KEYS = [e.name for e in tc.MATRIX if e.expect["hash_key"].takes]
# one entry per decode kind for the other scan modes: DEC128 -> 2, NARROW 8 -> 4, COPY of a decimal32, DATE64, MUL_I32, MUL_I64,
# DIV_I64, HALF_FLOAT, BOOL8, UUID, STRVIEW, and RUN_END over 8-byte and over 1-byte values
REPRESENTATIVES = ["dec128_4", "dec64_9", "dec32_9", "date64", "time32_s", "ts_s_utc", "ts_ns_utc", "f16", "bool8", "uuid", "string_view", "ree_ts_ns", "ree_bool8"]


@pytest.fixture(scope="module")
def con():
    return da.Connection(0)


class Fixture:
    pass


def _write(path, schema, batches, **options):
    with ipc.new_stream(path, schema, options=ipc.IpcWriteOptions(**options) if options else None) as w:
        for b in batches:
            w.write_batch(b)
    assert [b.num_rows for b in ipc.open_stream(path)] == list(tc.BATCHES)


@pytest.fixture(scope="module")
def fx(tmp_path_factory):
    f = Fixture()
    d = tmp_path_factory.mktemp("agg_types")
    files, f.stored = tc.tables()
    f.path = {}
    for name, (schema, batches) in files.items():
        f.path[name] = str(d / (name + ".arrows"))
        _write(f.path[name], schema, batches)
    for codec in ("lz4", "zstd"):
        f.path[codec] = str(d / (codec + ".arrows"))
        _write(f.path[codec], *files["main"], compression=codec)
    return f


def k9_specs(e):
    c = e.name
    if e.cls == tc.WIDE:
        return [("count", c), ("min", c), ("max", c), ("count_star",)]
    if e.cls == tc.FLOAT:       # (the constants keep every term exact: 2 v)
        return [("count", c), ("sum", c), ("min", c), ("max", c), ("sum_product", c, "pf"), ("sum_expr", (c, 4.0, 0.0), 0.5), ("count_star",)]
    return [("count", c), ("sum", c), ("min", c), ("max", c), ("sum_product", c, "p32"), ("sum_expr", (c, 3, -7), 5), ("count_star",)]


def want_of(e, spec, stored, rows):
    kind, value = tc.expected(spec, stored, rows)
    if e.duck == "UUID" and spec[0] in ("min", "max"):
        value = e.key_out(value)            # MIN / MAX of a UUID column come back as uuid.UUID
    return kind, value


def grouped_by_g(e, specs, stored, rows):
    """[(g, [want_of(spec) over the rows of the group])] ascending, the NULL group last"""
    members = {}
    for r in rows:
        members.setdefault(stored["g"][r], []).append(r)
    return [(k, [want_of(e, sp, stored, members[k]) for sp in specs]) for k in sorted(members, key=tc.order_key)]


def open_scan(con, path, expr, mode):
    rel = con.read_arrow(path, **mode)
    return rel.filter(expr) if expr is not None else rel


def run_k9(con, fx, e, path=None, modes=MODES[:1], runs=RUNS):
    specs = k9_specs(e)
    if e.cls == tc.FLOAT:        # once more behind the edge rows: every term finite, every sum held to the bound
        runs = runs + [("behind the non-finite edge rows", tc.FINITE_FILTER, tc.FINITE_ROWS)]
        assert all(v is None or math.isfinite(v) for v in fx.stored[e.name][800:])
    for what, expr, rows in runs:
        want = [want_of(e, sp, fx.stored, rows) for sp in specs]
        for mode in modes:
            got, scanned, selected = open_scan(con, path or fx.path[e.file], expr, mode).aggregate(specs, detail=True)
            assert (scanned, selected) == (N, len(rows)), (e.name, what, mode)
            for sp, g, w in zip(specs, got, want):
                tc.check(g, w, (e.name, what, mode, sp))


def check_groups(e_key, got, want, what):
    """got: [((key,), [values])] of the library; want: [(stored key, [expected])]; e_key: the key's entry (None: the int16 column)"""
    assert [g[0] for g in got] == [(e_key.key_out(k) if e_key else k,) for k, _ in want], (what, [g[0] for g in got][:8], [k for k, _ in want][:8])
    for (gk, gv), (wk, wv) in zip(got, want):
        assert len(gv) == len(wv)
        for g, w in zip(gv, wv):
            tc.check(g, w, (what, wk))


def run_k10_key(con, fx, e, path=None, modes=MODES[:1], runs=RUNS):
    low = e.low
    specs = [("count_star",), ("sum", "k"), ("min", "k"), ("max", "k")]
    for what, expr, rows in runs:
        want = tc.expected_groups(low.name, specs, fx.stored, rows)
        assert (want[-1][0] is None) == (None in low.stored) and 2 <= len(want) <= 4096
        for mode in modes:
            got, scanned, selected = open_scan(con, path or fx.path[e.file], expr, mode).group_aggregate([low.name], specs, detail=True)
            assert (scanned, selected) == (N, len(rows)), (e.name, what, mode)
            check_groups(low, got, want, (e.name, "K10 key", what, mode))


def run_k11_key(con, fx, e, path=None, modes=MODES[:1], runs=RUNS):
    specs = [("count_star",), ("sum", "k"), ("min", "k"), ("max", "k")]
    for what, expr, rows in runs:
        want = tc.expected_groups(e.name, specs, fx.stored, rows)
        assert (want[-1][0] is None) == (None in e.stored) and len(want) < HASH_GROUPS
        for mode in modes:
            got, scanned, selected = open_scan(con, path or fx.path[e.file], expr, mode).hash_aggregate(e.name, specs, HASH_GROUPS, detail=True)
            assert (scanned, selected) == (N, len(rows)), (e.name, what, mode)
            check_groups(e, got, want, (e.name, "K11 key", what, mode))


def refused(con, path, call, words, code=_ffi.MI_ENOTSUP, **options):
    """call(relation) raises MiError `code` whose message holds every word; the relation is closed here"""
    rel = con.read_arrow(path, **options)
    try:
        with pytest.raises(da.MiError) as x:
            call(rel)
    finally:
        rel.close()
    assert x.value.code == code, (words, x.value.code, str(x.value))
    for w in words:
        assert w in str(x.value), (w, str(x.value))
    return str(x.value)


# ------------------------------------------------------------------------------------------------ K9
@pytest.mark.parametrize("name", TAKEN_BY_K9)
def test_k9_aggregates_of_every_taken_type(con, fx, name):
    e = tc.BY_NAME[name]
    run_k9(con, fx, e)
    if e.cls == tc.WIDE:         # SUM over 16-byte values is the documented refusal; the connection goes on
        for spec in (("sum", name), ("sum_product", name, "p32"), ("sum_expr", (name, 1, 0), 2)):
            refused(con, fx.path[e.file], lambda rel: rel.aggregate([spec]), ("'%s'" % name, "(%s)" % e.duck, spec[0].upper()))
        assert con.read_arrow(fx.path[e.file]).aggregate([("count", name)]) == [tc.expected(("count", name), fx.stored, range(N))[1]]


@pytest.mark.parametrize("name", REFUSED_BY_K9)
def test_k9_refusals_name_the_column_and_its_type_and_count_still_works(con, fx, name):
    e = tc.BY_NAME[name]
    path = fx.path[e.file]
    for op in ("sum", "min", "max"):
        refused(con, path, lambda rel: rel.aggregate([(op, name)]), e.expect["aggregate"].words + (op.upper(),))
    refused(con, path, lambda rel: rel.aggregate([("sum_product", "p32", name)]), e.expect["aggregate"].words)
    if not e.count_works:
        refused(con, path, lambda rel: rel.aggregate([("count", name)]), e.expect["aggregate"].words + ("COUNT",))
        assert con.read_arrow(path).aggregate([("count_star",), ("max", "k")]) == [N, N - 1]
        return
    for what, expr, rows in RUNS:
        specs = [("count", name), ("count_star",), ("sum", "k")]
        got = open_scan(con, path, expr, MODES[0]).aggregate(specs)
        assert got == [tc.expected(sp, fx.stored, rows)[1] for sp in specs], (name, what)


# ------------------------------------------------------------------------------------------------ K10
@pytest.mark.parametrize("name", TAKEN_BY_K9)
def test_k10_aggregate_column_grouped_by_the_int16_column(con, fx, name):
    e = tc.BY_NAME[name]
    specs = k9_specs(e)
    for what, expr, rows in RUNS:
        want = grouped_by_g(e, specs, fx.stored, rows)
        assert len(want) == 41
        got, scanned, selected = open_scan(con, fx.path[e.file], expr, MODES[0]).group_aggregate(["g"], specs, detail=True)
        assert (scanned, selected) == (N, len(rows))
        check_groups(None, got, want, (name, "K10 column", what))


@pytest.mark.parametrize("name", K10_KEYS)
def test_k10_key_of_every_taken_type(con, fx, name):
    e = tc.BY_NAME[name]
    if not e.long_key:
        run_k10_key(con, fx, e)
        return
    # fixed_size_binary(13): a selected valid row has no inline image; with those rows deselected the same call answers
    specs = [("count_star",), ("sum", "k")]
    for expr in (None, tc.FILTER):
        refused(con, fx.path[e.file], lambda rel: (rel.filter(expr) if expr else rel).group_aggregate([name], specs),
                ("a VARCHAR / BLOB group key longer than 12 bytes stays above the scan",))
    rows = [r for r in range(N) if fx.stored[name][r] is None]
    got, scanned, selected = con.read_arrow(fx.path[e.file]).filter((name, "is null")).group_aggregate([name], specs, detail=True)
    assert (scanned, selected) == (N, len(rows)) and got == [((None,), [len(rows), sum(rows)])]


@pytest.mark.parametrize("name", [e.name for e in tc.MATRIX if not e.expect["group_key"].takes])
def test_k10_and_k11_key_refusals_and_a_good_query_follows(con, fx, name):
    e = tc.BY_NAME[name]
    path = fx.path[e.file]
    refused(con, path, lambda rel: rel.group_aggregate([name], [("count_star",)]), e.expect["group_key"].words)
    refused(con, path, lambda rel: rel.group_aggregate(["g", name], [("count_star",)]), e.expect["group_key"].words)
    refused(con, path, lambda rel: rel.hash_aggregate(name, [("count_star",)], HASH_GROUPS), e.expect["hash_key"].words)
    want = tc.expected_groups("g", [("count_star",)], fx.stored, range(N))
    check_groups(None, con.read_arrow(path).group_aggregate(["g"], [("count_star",)]), want, "after the refusals")
    check_groups(None, con.read_arrow(path).hash_aggregate("g", [("count_star",)], 64), want, "after the refusals")


# ------------------------------------------------------------------------------------------------ K11
@pytest.mark.parametrize("name", K11_KEYS)
def test_k11_key_of_every_integer_like_type(con, fx, name):
    run_k11_key(con, fx, tc.BY_NAME[name])


@pytest.mark.parametrize("name", TAKEN_BY_K9)
def test_k11_aggregate_column_grouped_by_the_int16_column(con, fx, name):
    e = tc.BY_NAME[name]
    path = fx.path[e.file]
    good = {tc.WIDE: [("count", name), ("count_star",)], tc.FLOAT: [("count", name), ("min", name), ("max", name), ("count_star",)]}.get(e.cls, k9_specs(e))
    if e.cls == tc.FLOAT:        # the table adds in arrival order: no floating-point sum
        for spec in (("sum", name), ("sum_product", name, "pf"), ("sum_expr", (name, 4.0, 0.0), 0.5)):
            refused(con, path, lambda rel: rel.hash_aggregate("g", [spec], 64), ("'%s'" % name, "(%s)" % e.duck, spec[0].upper(), "floating-point sum"))
    if e.cls == tc.WIDE:         # no 128-bit atomic: no MIN / MAX of 16-byte values; SUM as in K9
        for op in ("min", "max"):
            refused(con, path, lambda rel: rel.hash_aggregate("g", [(op, name)], 64), ("'%s'" % name, "(%s)" % e.duck, op.upper(), "no 128-bit atomic"))
        refused(con, path, lambda rel: rel.hash_aggregate("g", [("sum", name)], 64), ("'%s'" % name, "(%s)" % e.duck, "SUM"))
    for what, expr, rows in RUNS:
        want = grouped_by_g(e, good, fx.stored, rows)
        got, scanned, selected = open_scan(con, path, expr, MODES[0]).hash_aggregate("g", good, 64, detail=True)
        assert (scanned, selected) == (N, len(rows))
        check_groups(None, got, want, (name, "K11 column", what))


@pytest.mark.parametrize("name", [e.name for e in tc.MATRIX if e.expect["group_key"].takes and not e.expect["hash_key"].takes])
def test_k11_refuses_wide_and_string_keys_that_k10_takes(con, fx, name):
    e = tc.BY_NAME[name]
    path = fx.path[e.file]
    refused(con, path, lambda rel: rel.hash_aggregate(e.low.name, [("count_star",)], HASH_GROUPS),
            tuple(w.replace(name, e.low.name) for w in e.expect["hash_key"].words) + ("mi_scan_group_aggregate takes",))
    got = con.read_arrow(path).hash_aggregate("g", [("count_star",)], 64)
    check_groups(None, got, tc.expected_groups("g", [("count_star",)], fx.stored, range(N)), "after the refusal")


# ------------------------------------------------------------------------------------------------ scan modes, compressed bodies
@pytest.mark.parametrize("name", REPRESENTATIVES)
def test_one_entry_per_decode_kind_in_the_other_scan_modes(con, fx, name):
    """a host consumer, and zero_copy_direct with unset_all_valid (device-resident and not)"""
    e = tc.BY_NAME[name]
    filtered = RUNS[1:]
    if e.expect["aggregate"].takes:
        run_k9(con, fx, e, modes=MODES[1:], runs=filtered)
    if e.expect["group_key"].takes:
        run_k10_key(con, fx, e, modes=MODES[1:], runs=filtered)
    if e.expect["hash_key"].takes:
        run_k11_key(con, fx, e, modes=MODES[1:], runs=filtered)


@pytest.mark.parametrize("name", [e.name for e in tc.TWINS])
def test_twins_without_nulls_in_every_scan_mode(con, fx, name):
    """the column a zero_copy_direct scan aliases into the body (a copied decimal64) and one it must not (a narrowed
    decimal128), with no validity words under unset_all_valid"""
    e = tc.BY_NAME[name]
    assert None not in e.stored
    rel = con.read_arrow(fx.path["main"], **MODES[2])
    assert rel.aggregate([("sum", name)]) == [sum(e.stored)]
    assert rel.stats()["aliased_bytes"] == (N * 8 if name == "dec64_18_nn" else 0)       # aliased where the decode is a copy, only there
    rel.close()
    run_k9(con, fx, e, modes=MODES)
    run_k10_key(con, fx, e, modes=MODES, runs=RUNS[1:])
    run_k11_key(con, fx, e, modes=MODES, runs=RUNS[1:])


@pytest.mark.parametrize("codec", ["lz4", "zstd"])
def test_a_narrowed_decimal_from_compressed_bodies(con, fx, codec):
    e = tc.BY_NAME["dec128_4"]
    run_k9(con, fx, e, path=fx.path[codec], modes=MODES[:2])
    run_k10_key(con, fx, e, path=fx.path[codec], modes=MODES[:2], runs=RUNS[1:])
    run_k11_key(con, fx, e, path=fx.path[codec], modes=MODES[:2], runs=RUNS[1:])


# ------------------------------------------------------------------------------------------------ a decode cast that overflows
def test_a_timestamp_whose_cast_to_microseconds_overflows_fails_the_call_and_under_a_null_does_not(con, tmp_path):
    """timestamp[s, UTC] * 10^6: 9223372036855 s is the first value that does not fit.  A status flag, not a fault."""
    n, bad = 3000, 2500
    rng = np.random.default_rng(5)
    raws = [int(v) for v in rng.integers(-4 * 10 ** 9, 4 * 10 ** 9, n)]
    raws[bad] = 9223372036855
    raws[7] = 9223372036854
    everything = np.ones(n, bool)
    specs = [("count", "t"), ("sum", "t"), ("min", "t"), ("max", "t"), ("count_star",)]
    for null_at_bad in (False, True):
        ok = everything.copy()
        ok[::9] = False
        ok[bad] = not null_at_bad
        ok[7] = True
        t = tc._fixed(pa.timestamp("s", tz="UTC"), tc._le(raws, 8, everything), ok)     # (the value stays in the buffer under the NULL)
        table = pa.table({"k": pa.array(np.arange(n, dtype=np.int64)), "g": pa.array((np.arange(n) % 5).astype(np.int16)), "t": t})
        path = str(tmp_path / ("overflow_%d.arrows" % null_at_bad))
        with ipc.new_stream(path, table.schema) as w:
            w.write_table(table)
        if not null_at_bad:
            for call in (lambda rel: rel.aggregate(specs), lambda rel: rel.group_aggregate(["g"], specs), lambda rel: rel.hash_aggregate("t", [("count_star",)], 4096)):
                rel = con.read_arrow(path)
                try:
                    with pytest.raises(da.MiError) as x:
                        call(rel)
                finally:
                    rel.close()
                assert "Could not convert Timestamp to Microsecond" in str(x.value), str(x.value)
            continue
        stored = dict(t=[r * 10 ** 6 if o else None for r, o in zip(raws, ok)], k=list(range(n)))
        got = con.read_arrow(path).aggregate(specs)
        for sp, g in zip(specs, got):
            tc.check(g, tc.expected(sp, stored, range(n)), ("the overflowing value under a NULL", sp))
        assert got[3] == 9223372036854 * 10 ** 6
        rows = con.read_arrow(path).hash_aggregate("t", [("count_star",)], 4096)
        assert len(rows) == len(set(stored["t"])) and rows[-1] == ((None,), [stored["t"].count(None)])


# ------------------------------------------------------------------------------------------------ types outside the matrix
OTHERS = {"lst": "INTEGER[]", "st": "STRUCT(x BIGINT, y VARCHAR)", "mp": "MAP(INTEGER, VARCHAR)", "un": "UNION(a BIGINT, b VARCHAR)", "dct": "VARCHAR",
          "f32key": "FLOAT", "filename": "VARCHAR"}


@pytest.fixture(scope="module")
def others(tmp_path_factory):
    n = 3000
    rng = np.random.default_rng(6)
    arrays = {"k": pa.array(np.arange(n, dtype=np.int64)), "g": pa.array(rng.integers(0, 5, n).astype(np.int16))}
    arrays["lst"] = pa.array([[i % 3] for i in range(n)], pa.list_(pa.int32()))
    arrays["st"] = pa.array([{"x": i, "y": str(i % 7)} for i in range(n)], pa.struct([("x", pa.int64()), ("y", pa.string())]))
    arrays["mp"] = pa.array([[(i % 3, "v")] for i in range(n)], pa.map_(pa.int32(), pa.string()))
    arrays["un"] = pa.UnionArray.from_sparse(pa.array(np.zeros(n, np.int8)), [pa.array(np.arange(n, dtype=np.int64)), pa.array(["u"] * n)], ["a", "b"])
    arrays["dct"] = pa.array([("x", "y")[i] for i in rng.integers(0, 2, n)], pa.string()).dictionary_encode()
    arrays["f32key"] = pa.array(rng.integers(0, 3, n).astype(np.float32))
    table = pa.table(arrays)
    path = str(tmp_path_factory.mktemp("agg_types_others") / "others.arrows")
    with ipc.new_stream(path, table.schema) as w:
        w.write_table(table)
    return path, n, [int(v) for v in arrays["g"].to_pylist()]


@pytest.mark.parametrize("name", list(OTHERS))
def test_nested_union_dictionary_float_key_and_constant_columns_are_refused_by_name_and_type(con, others, name):
    path, n, g = others
    typed = "'%s' (%s)" % (name, OTHERS[name])
    options = dict(accept_dictionaries=True, filename=(name == "filename"))
    refused(con, path, lambda rel: rel.group_aggregate([name], [("count_star",)]), (typed, "GROUP BY"), **options)
    refused(con, path, lambda rel: rel.hash_aggregate(name, [("count_star",)], 64), (typed, "GROUP BY"), **options)
    if name != "f32key":
        refused(con, path, lambda rel: rel.aggregate([("max", name)]), (typed, "MAX"), **options)
    else:
        assert con.read_arrow(path, **options).aggregate([("max", name)]) == [2.0]
    if name in ("un", "dct", "filename"):       # no aggregate reads these, COUNT included
        refused(con, path, lambda rel: rel.aggregate([("count", name)]), (typed, "COUNT"), **options)
    counts = [((k,), [g.count(k)]) for k in sorted(set(g))]
    assert con.read_arrow(path, **options).group_aggregate(["g"], [("count_star",)]) == counts
    assert con.read_arrow(path, **options).hash_aggregate("g", [("count_star",)], 64) == counts
    assert con.read_arrow(path, **options).aggregate([("count_star",), ("max", "k")]) == [n, n - 1]
