"""mi_scan_hash_aggregate end to end: GROUP BY one integer key with thousands of groups over files written by pyarrow --
under filters, for host and device-resident consumers, compressed bodies, two files, a run-end encoded key, rank / world
and two contexts -- and the TPC-H shapes `group by l_orderkey` / `l_suppkey` on the synthetic lineitem.  Results are held
to the dict loop of hash_agg_cases.py over pyarrow's reading of the file, and to pyarrow's group_by where it can express
the aggregate.  Expected values never come from the library."""
import ctypes as C
import decimal
import os
import subprocess

import numpy as np
import pyarrow as pa
import pyarrow.ipc as ipc
import pytest

import duckdb_arrow_amd as da
from duckdb_arrow_amd import _ffi

import hash_agg_cases as hc
from test_gpu_scan_aggregate import _read_back

pytestmark = pytest.mark.gpu

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
CTX = decimal.Context(prec=60)
N = 15000
BATCH_ROWS = 5000
MAX_GROUPS = 16384
MODES = [dict(device_resident=True), dict(), dict(device_resident=True, unset_all_valid=True, zero_copy_direct=True)]
SPECS = [("count_star",), ("count", "dec"), ("sum", "i64"), ("sum", "dec"), ("sum_product", "i32", "i64"), ("min", "f64"), ("max", "f64"),
         ("sum_expr", ("dec", 2, -1), "i32", 3)]
PA_SPECS = [("count_star",), ("count", "dec"), ("sum", "i64"), ("min", "i32"), ("max", "i32")]
PA_AGGS = [([], "count_all"), ("dec", "count"), ("i64", "sum"), ("i32", "min"), ("i32", "max")]


@pytest.fixture(scope="module")
def con():
    return da.Connection(0)


def host_columns(py):
    """pyarrow's reading of a file (stored values, None for NULL) as the case module's columns"""
    cols = {}
    for name, values in py.items():
        live = [v for v in values if v is not None]
        if not live or isinstance(live[0], bool) or not isinstance(live[0], (int, float)):
            continue
        if isinstance(live[0], float):
            cols[name] = hc.HostColumn(np.array([0.0 if v is None else v for v in values]), "float", [v is not None for v in values])
        elif max(abs(v) for v in live) < 1 << 63:
            cols[name] = hc.HostColumn(np.array([0 if v is None else v for v in values], np.int64), "signed", [v is not None for v in values])
    return cols


def by_name(cols, specs):
    def arg(a):
        if isinstance(a, str):
            return cols[a]
        if isinstance(a, tuple) and isinstance(a[0], str):
            return (cols[a[0]],) + tuple(a[1:])
        return a
    return [(sp[0],) + tuple(arg(a) for a in sp[1:]) for sp in specs]


def check(got, want, what=""):
    """`got` as Relation.hash_aggregate returns it, `want` as hc.reference does"""
    assert [g[0][0] for g in got] == [w[0] for w in want], (what, [g[0] for g in got][:6], [w[0] for w in want][:6])
    for (gk, gv), (wk, wv) in zip(got, want):
        assert len(gv) == len(wv) and all(hc.same_value(g, w[0]) for g, w in zip(gv, wv)), (what, wk, gv, wv)


class Fixture:
    pass


def _table(rng, n, first_key=0):
    mask = lambda p=0.12: rng.random(n) < p
    k = (rng.integers(0, 13000, n) + first_key) * 1000003 - 5 * 10 ** 9
    k[5] = -1                                                   # the table's empty mark as a key
    k[6] = -2
    arrays = {"k": pa.array(k.astype(np.int64), mask=mask(0.04))}
    arrays["row"] = pa.array(np.arange(n, dtype=np.int64))
    arrays["i64"] = pa.array(rng.integers(-(1 << 40), 1 << 40, n), mask=mask())
    arrays["i32"] = pa.array(rng.integers(-1000, 1000, n).astype(np.int32), mask=mask())
    arrays["dec"] = pa.array([None if x else CTX.scaleb(decimal.Decimal(int(v)), -2) for v, x in zip(rng.integers(-10 ** 14, 10 ** 14, n), mask())], pa.decimal128(15, 2))
    f = rng.normal(0, 1e4, n) * rng.choice([1e-6, 1.0, 1e6], n)
    f[rng.integers(0, n, 300)] = np.array([np.nan, np.inf, -np.inf, -0.0])[rng.integers(0, 4, 300)]
    arrays["f64"] = pa.array(f, mask=mask())
    arrays["s"] = pa.array([None if x else ("MAIL", "SHIP", "", "REG AIR")[i] for i, x in zip(rng.integers(0, 4, n), mask())], pa.string())
    arrays["k16"] = pa.array((rng.integers(0, 3000, n) - 1500).astype(np.int16))
    arrays["b"] = pa.array(rng.random(n) < 0.5, mask=mask())
    return arrays


@pytest.fixture(scope="module")
def fx(tmp_path_factory):
    rng = np.random.default_rng(1811)
    arrays = _table(rng, N)
    arrays["hug"] = pa.array([decimal.Decimal(int(v)) for v in rng.integers(0, 50, N)], pa.decimal128(38, 0))
    arrays["d"] = pa.array([("x", "y")[i] for i in rng.integers(0, 2, N)], pa.string()).dictionary_encode()
    arrays["un"] = pa.UnionArray.from_sparse(pa.array(np.zeros(N, np.int8)), [pa.array(np.arange(N, dtype=np.int64)), pa.array(["u"] * N)])
    table = pa.table(arrays)
    f = Fixture()
    f.dir = tmp_path_factory.mktemp("hashagg")
    f.path = str(f.dir / "t.arrows")
    with ipc.new_stream(f.path, table.schema) as w:
        w.write_table(table, max_chunksize=BATCH_ROWS)
    assert [b.num_rows for b in ipc.open_stream(f.path)] == [5000, 5000, 5000]
    f.table = table
    f.py = _read_back(f.path)
    f.cols = host_columns(f.py)
    f.want = hc.reference(f.cols["k"], by_name(f.cols, SPECS), range(N))
    assert 8000 < len(f.want) < 10000 and f.want[-1][0] is None and -1 in [w[0] for w in f.want]
    return f


FILTERS = {
    "none": (None, lambda py, r: True),
    "integer": (("and", ("i32", ">=", -500), ("i32", "<", 700)), lambda py, r: py["i32"][r] is not None and -500 <= py["i32"][r] < 700),
    "string": (("s", "=", "SHIP"), lambda py, r: py["s"][r] == "SHIP"),
}


@pytest.mark.parametrize("name", list(FILTERS))
def test_thousands_of_groups_under_filters_for_host_and_device_consumers(con, fx, name):
    expr, keep = FILTERS[name]
    rows = [r for r in range(N) if keep(fx.py, r)]
    assert 0 < len(rows) <= N and (expr is None or len(rows) < N)
    want = fx.want if expr is None else hc.reference(fx.cols["k"], by_name(fx.cols, SPECS), rows)
    results = []
    for mode in MODES:
        rel = con.read_arrow(fx.path, accept_dictionaries=True, **mode)
        got, scanned, selected = (rel.filter(expr) if expr is not None else rel).hash_aggregate("k", SPECS, MAX_GROUPS, detail=True)
        assert (scanned, selected) == (N, len(rows)), (name, mode)
        check(got, want, (name, mode))
        results.append(repr(got))
    assert results[0] == results[1] == results[2]
    # filter_compact is ignored
    rel = con.read_arrow(fx.path, accept_dictionaries=True, filter_compact=True)
    assert repr((rel.filter(expr) if expr is not None else rel).hash_aggregate("k", SPECS, MAX_GROUPS)) == results[0]


def test_against_pyarrow_group_by(con, fx):
    want_pa = hc.pyarrow_groups(fx.table, "k", PA_AGGS)
    got = con.read_arrow(fx.path, accept_dictionaries=True).hash_aggregate("k", PA_SPECS, MAX_GROUPS)
    assert [(k[0], v) for k, v in got] == want_pa
    check(got, hc.reference(fx.cols["k"], by_name(fx.cols, PA_SPECS), range(N)), "pyarrow's specs")


def test_the_gap_group_aggregate_still_refuses_this_file(con, fx):
    rel = con.read_arrow(fx.path, accept_dictionaries=True)
    try:
        with pytest.raises(da.MiError) as e:
            rel.group_aggregate(["k"], [("count_star",)])
    finally:
        rel.close()
    assert e.value.code == _ffi.MI_ENOTSUP and "GROUP BY with more than" in str(e.value) and "stays above the scan" in str(e.value)


@pytest.mark.parametrize("codec", ["lz4", "zstd"])
def test_compressed_bodies(con, fx, codec):
    path = str(fx.dir / ("t_%s.arrows" % codec))
    with ipc.new_stream(path, fx.table.schema, options=ipc.IpcWriteOptions(compression=codec)) as w:
        w.write_table(fx.table, max_chunksize=BATCH_ROWS)
    for mode in MODES[:2]:
        check(con.read_arrow(path, accept_dictionaries=True, **mode).hash_aggregate("k", SPECS, MAX_GROUPS), fx.want, (codec, mode))


def test_two_files(con, fx, tmp_path):
    rng = np.random.default_rng(99)
    other = pa.table(_table(rng, 6000, first_key=9000)).select(["k", "row", "i64", "i32", "dec", "f64", "s"])
    path = str(tmp_path / "other.arrows")
    with ipc.new_stream(path, other.schema) as w:
        w.write_table(other, max_chunksize=2500)
    py = {name: fx.py[name] + more for name, more in _read_back(path).items()}
    cols = host_columns(py)
    want = hc.reference(cols["k"], by_name(cols, SPECS), range(N + 6000))
    assert len(want) > len(fx.want)
    got, scanned, selected = con.read_arrow([fx.path, path], union_by_name=True, accept_dictionaries=True).hash_aggregate("k", SPECS, MAX_GROUPS, detail=True)
    assert scanned == selected == N + 6000
    check(got, want, "two files")


def test_a_run_end_encoded_key_column(con, tmp_path):
    rng = np.random.default_rng(8)
    n, per_batch = 12000, 4000
    path = str(tmp_path / "ree.arrows")
    schema = pa.schema([("r", pa.run_end_encoded(pa.int32(), pa.int64())), ("v", pa.int64())])
    with ipc.new_stream(path, schema) as w:
        for first in range(0, n, per_batch):
            ends = np.cumsum(rng.integers(1, 3, per_batch))
            ends = ends[ends < per_batch].tolist() + [per_batch]
            values = [None if rng.random() < 0.05 else int(v) for v in rng.integers(-4000, 4000, len(ends))]
            ree = pa.RunEndEncodedArray.from_arrays(pa.array(ends, pa.int32()), pa.array(values, pa.int64()))
            w.write_batch(pa.record_batch([ree, pa.array(np.arange(first, first + per_batch, dtype=np.int64))], schema=schema))
    cols = host_columns(_read_back(path))
    specs = [("count_star",), ("sum", "v"), ("max", "v"), ("count", "r")]
    for expr, rows in ((None, list(range(n))), (("v", ">=", 2500), list(range(2500, n)))):
        want = hc.reference(cols["r"], by_name(cols, specs), rows)
        assert len(want) > 4096 or expr is not None
        for mode in MODES[:2]:
            rel = con.read_arrow(path, **mode)
            check((rel.filter(expr) if expr else rel).hash_aggregate("r", specs, 8192), want, ("ree", expr, mode))


def _merge(parts, specs):
    """rank lists -> one, merged in the test by key with the rules of SQL"""
    merged = {}
    for part in parts:
        for (key,), values in part:
            if key not in merged:
                merged[key] = list(values)
                continue
            for i, (sp, v) in enumerate(zip(specs, values)):
                old = merged[key][i]
                if v is None or old is None:
                    merged[key][i] = v if old is None else old
                elif sp[0] in ("min", "max"):
                    pick = min if sp[0] == "min" else max
                    merged[key][i] = hc.canonical(pick(old, v, key=hc.float_order)) if isinstance(v, float) else pick(old, v)
                else:
                    merged[key][i] = old + v if sp[0] in ("count", "count_star") else hc.wrap128(old + v)
    return [((k,), merged[k]) for k in sorted(merged, key=hc.order_key)]


def test_rank_world_shares_and_two_contexts_equal_the_whole(con, fx):
    expr = ("i32", "<", 600)
    rows = [r for r in range(N) if fx.py["i32"][r] is not None and fx.py["i32"][r] < 600]
    want = hc.reference(fx.cols["k"], by_name(fx.cols, SPECS), rows)
    whole = con.read_arrow(fx.path, accept_dictionaries=True).filter(expr).hash_aggregate("k", SPECS, MAX_GROUPS)
    check(whole, want, "whole")
    rel = con.read_arrow(fx.path, accept_dictionaries=True, contexts=[da.Context(0), da.Context(0)], device_resident=True).filter(expr)
    got, scanned, selected = rel.hash_aggregate("k", SPECS, MAX_GROUPS, detail=True)
    assert (scanned, selected) == (N, len(rows)) and repr(got) == repr(whole)
    parts = [con.read_arrow(fx.path, accept_dictionaries=True, rank=r, world=2).filter(expr).hash_aggregate("k", SPECS, MAX_GROUPS, detail=True) for r in range(2)]
    assert sum(p[1] for p in parts) == N and sum(p[2] for p in parts) == len(rows)
    assert all(0 < len(p[0]) < len(want) for p in parts)
    assert repr(_merge([p[0] for p in parts], SPECS)) == repr(whole)
    # the devices' lists together may not exceed max_groups either
    rel = con.read_arrow(fx.path, accept_dictionaries=True, contexts=[da.Context(0), da.Context(0)], device_resident=True).filter(expr)
    try:
        with pytest.raises(da.MiError) as e:
            rel.hash_aggregate("k", [("count_star",)], max(len(p[0]) for p in parts) + 200)
    finally:
        rel.close()
    assert e.value.code == _ffi.MI_ENOTSUP and "max_groups" in str(e.value)


@pytest.fixture(scope="module")
def lineitem(tmp_path_factory):
    buf, info = da.synth_lineitem_stream(scale_factor=1.0, seed=21, n_rows=7000, rows_per_batch=3000)
    f = Fixture()
    f.path = str(tmp_path_factory.mktemp("hashagg_li") / "lineitem.arrows")
    buf.tofile(f.path)
    f.py = _read_back(f.path)
    f.cols = host_columns(f.py)
    f.n = info["n_rows"]
    return f


TPCH = [("sum", "l_quantity"), ("count_star",), ("min", "l_shipdate"), ("max", "l_extendedprice"), ("sum_expr", "l_extendedprice", ("l_discount", -1, 100)),
        ("count", "l_comment")]


@pytest.mark.parametrize("key", ["l_orderkey", "l_suppkey"])
def test_tpch_shapes_on_the_synthetic_lineitem(con, lineitem, key):
    specs = [sp for sp in TPCH if sp[0] != "count"]      # (the reference's columns are the numeric ones)
    want = hc.reference(lineitem.cols[key], by_name(lineitem.cols, specs), range(lineitem.n))
    assert len(want) > 1000
    for mode in MODES[:2]:
        got, scanned, selected = con.read_arrow(lineitem.path, **mode).hash_aggregate(key, specs, 8192, detail=True)
        assert scanned == selected == lineitem.n
        check(got, want, (key, mode))
    # Q18's inner query with its filter pushed down as well: orders of 1995 and later lines only
    expr = ("l_shipdate", ">=", 9131)
    rows = [r for r in range(lineitem.n) if lineitem.py["l_shipdate"][r] is not None and lineitem.py["l_shipdate"][r] >= 9131]
    check(con.read_arrow(lineitem.path).filter(expr).hash_aggregate(key, specs, 8192), hc.reference(lineitem.cols[key], by_name(lineitem.cols, specs), rows), "filtered")
    # a COUNT of a string column rides along
    got = con.read_arrow(lineitem.path).hash_aggregate(key, TPCH, 8192)
    assert [v[:5] for _, v in got] == [[x[0] for x in w[1]] for w in want] and all(v[5] <= v[1] for _, v in got)


def test_max_groups_too_small_names_it_and_capacity_too_small_sets_the_count(con, fx):
    distinct = len(fx.want)
    for max_groups in (1, 4096, distinct - 1):
        rel = con.read_arrow(fx.path, accept_dictionaries=True)
        try:
            with pytest.raises(da.MiError) as e:
                rel.hash_aggregate("k", [("count_star",)], max_groups)
        finally:
            rel.close()
        assert e.value.code == _ffi.MI_ENOTSUP and "max_groups = %d" % max_groups in str(e.value), str(e.value)
    assert len(con.read_arrow(fx.path, accept_dictionaries=True).hash_aggregate("k", [("count_star",)], distinct)) == distinct
    rel = con.read_arrow(fx.path, accept_dictionaries=True)
    with pytest.raises(da.MiError) as e:
        rel.hash_aggregate("k", [("count_star",)], MAX_GROUPS, capacity=100)
    rel.close()
    assert e.value.code == _ffi.MI_EINVAL and str(distinct) in str(e.value)
    rel = con.read_arrow(fx.path, accept_dictionaries=True)
    spec = (_ffi.AggSpec * 1)()
    spec[0].op = _ffi.AGG_COUNT_STAR
    out_k, out_v, n = (_ffi.GroupKeyValue * 8)(), (_ffi.AggValue * 8)(), C.c_int32(-1)
    assert _ffi.lib().mi_scan_hash_aggregate(rel._h, b"k", spec, 1, MAX_GROUPS, out_k, out_v, 8, C.byref(n), None, None) == _ffi.MI_EINVAL
    assert n.value == distinct
    for bad in (0, -5, (1 << 24) + 1):
        assert _ffi.lib().mi_scan_hash_aggregate(rel._h, b"k", spec, 1, bad, out_k, out_v, 8, C.byref(n), None, None) == _ffi.MI_EINVAL
        assert b"max_groups" in _ffi.lib().mi_last_error()
    rel.close()


def test_other_key_types(con, fx):
    """a 2-byte key, a BOOLEAN key (as bool), a key without NULLs"""
    for key in ("k16", "b", "row"):
        col = fx.cols.get(key) or hc.HostColumn(np.array([0 if v is None else int(v) for v in fx.py[key]], np.int64), "signed", [v is not None for v in fx.py[key]])
        want = hc.reference(col, by_name(fx.cols, SPECS), range(N))
        got = con.read_arrow(fx.path, accept_dictionaries=True).hash_aggregate(key, SPECS, MAX_GROUPS)
        if key == "b":
            assert [k[0] for k, _ in got] == [False, True, None]
            got = [((None if k[0] is None else int(k[0]),), v) for k, v in got]
        check(got, want, key)


def test_refusals_name_the_column_and_a_good_query_follows(con, fx):
    def refused(key, code, *words, specs=(("count_star",),), **options):
        rel = con.read_arrow(fx.path, accept_dictionaries=True, **options)
        try:
            with pytest.raises(da.MiError) as e:
                rel.hash_aggregate(key, list(specs), MAX_GROUPS)
        finally:
            rel.close()
        assert e.value.code == code, (key, e.value.code, str(e.value))
        for w in words:
            assert w in str(e.value), (key, w, str(e.value))

    refused(["k", "k16"], _ffi.MI_ENOTSUP, "ONE key column", "group_aggregate", "few groups")
    refused("hug", _ffi.MI_ENOTSUP, "'hug'", "a 16-byte key", "mi_scan_group_aggregate takes", "few groups")
    refused("s", _ffi.MI_ENOTSUP, "'s'", "a VARCHAR / BLOB key", "mi_scan_group_aggregate takes", "few groups")
    refused("f64", _ffi.MI_ENOTSUP, "'f64'", "stays above the scan")      # no grouped call takes a DOUBLE key: no pointer to K10
    rel = con.read_arrow(fx.path, accept_dictionaries=True)
    with pytest.raises(da.MiError) as e:
        rel.hash_aggregate("f64", [("count_star",)], MAX_GROUPS)
    rel.close()
    assert "mi_scan_group_aggregate" not in str(e.value)
    refused("d", _ffi.MI_ENOTSUP, "'d'", "GROUP BY", "dictionary")
    refused("un", _ffi.MI_ENOTSUP, "'un'", "GROUP BY", "union")
    refused("filename", _ffi.MI_ENOTSUP, "'filename'", "GROUP BY", "constant", filename=True)
    refused("nope", _ffi.MI_EINVAL, "'nope'")
    refused("k", _ffi.MI_ENOTSUP, "SUM", "'f64'", "arrival order", "mi_scan_group_aggregate", specs=[("sum", "f64")])
    refused("k", _ffi.MI_ENOTSUP, "SUM_PRODUCT", "'f64'", "arrival order", specs=[("count_star",), ("sum_product", "f64", "f64")])
    refused("k", _ffi.MI_ENOTSUP, "SUM_EXPR", "'f64'", "arrival order", specs=[("sum_expr", ("f64", 2.0, 1.0))])
    refused("k", _ffi.MI_ENOTSUP, "MIN", "'hug'", "128-bit atomic", specs=[("min", "hug")])
    refused("k", _ffi.MI_ENOTSUP, "MAX", "'hug'", "128-bit atomic", specs=[("max", "hug")])
    refused("k", _ffi.MI_ENOTSUP, "'s'", "SUM", specs=[("sum", "s")])
    # what K10 takes of these for few groups, it still takes
    assert len(con.read_arrow(fx.path, accept_dictionaries=True).group_aggregate(["hug"], [("sum", "f64"), ("min", "hug")])) == 50
    # after init
    rel = con.read_arrow(fx.path, accept_dictionaries=True).project(["k"])
    assert rel.count() == N
    try:
        with pytest.raises(da.MiError) as e:
            rel.hash_aggregate("k", [("count_star",)], MAX_GROUPS)
    finally:
        rel.close()
    assert e.value.code == _ffi.MI_EINVAL and "right after bind" in str(e.value)
    # the same Connection runs a good query, and the other calls still answer
    check(con.read_arrow(fx.path, accept_dictionaries=True).hash_aggregate("k", SPECS, MAX_GROUPS), fx.want, "after the refusals")
    assert con.read_arrow(fx.path, accept_dictionaries=True).aggregate([("count_star",)]) == [N]


def test_counters_count_one_launch_per_record_batch_and_one_collect(con, fx):
    before = da.hash_aggregate_counters()
    con.read_arrow(fx.path, accept_dictionaries=True).hash_aggregate("k", [("count_star",)], MAX_GROUPS)
    after = da.hash_aggregate_counters()
    assert (after[0] - before[0], after[1] - before[1]) == (3, 1)


def test_plain_c_client_applies_the_having_of_q18(lineitem, tmp_path):
    """examples/hash_agg.c: SELECT l_orderkey, sum(l_quantity), count(*) ... GROUP BY l_orderkey through the C ABI, HAVING by the client"""
    exe = str(tmp_path / "hash_agg")
    libdir = os.path.join(ROOT, "duckdb-arrow_amd")
    subprocess.run(["gcc", "-std=c99", "-Wall", "-Wextra", "-Werror", "-I" + os.path.join(ROOT, "include"), os.path.join(ROOT, "examples", "hash_agg.c"),
                    "-L" + libdir, "-lmi_arrow_ipc", "-Wl,-rpath," + libdir, "-o", exe], check=True, capture_output=True)
    want = hc.reference(lineitem.cols["l_orderkey"], by_name(lineitem.cols, [("sum", "l_quantity"), ("count_star",)]), range(lineitem.n))
    sums = sorted(w[1][0][0] for w in want if w[1][0][0] is not None)
    quantity = sums[len(sums) * 9 // 10] // 100          # a threshold that keeps about a tenth of the orders
    r = subprocess.run([exe, "-q", str(quantity), lineitem.path], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    lines = r.stdout.splitlines()
    assert lines[0] == "%d orders in %d rows" % (len(want), lineitem.n)
    kept = [(k, v[0][0], v[1][0]) for k, v in want if v[0][0] is not None and v[0][0] > quantity * 100]
    assert 0 < len(kept) < len(want) and lines[-1] == "%d orders with sum(l_quantity) > %d" % (len(kept), quantity)
    assert [ln.split() for ln in lines[2:-1]] == [["NULL" if k is None else str(k), "%d.%02d" % (s // 100, s % 100), str(c)] for k, s, c in kept]
