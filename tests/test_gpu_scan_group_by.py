"""mi_scan_group_aggregate end to end: GROUP BY over files, under every family of pushed-down filter, for host and
device-resident consumers, two contexts and rank / world, against the reference's known answer (`group by fruit`),
pyarrow's Table.group_by on the golden lineitem head, and a Python dict loop over pyarrow's reading of a written table.
Expected values never come from the library."""
import datetime
import decimal
import glob
import math
import os
import subprocess

import numpy as np
import pyarrow as pa
import pyarrow.compute as pc
import pyarrow.ipc as ipc
import pytest

import duckdb_arrow_amd as da
from duckdb_arrow_amd import _ffi
from test_gpu_scan_aggregate import _read_back, _wrap128

pytestmark = pytest.mark.gpu

HERE = os.path.dirname(os.path.abspath(__file__))
LINEITEM = os.path.join(HERE, "golden", "lineitem_sf0_01_head.arrows")
EPOCH = datetime.date(1970, 1, 1)
CTX = decimal.Context(prec=60)
N = 15000
BATCH_ROWS = 4000
MODES = [dict(device_resident=True), dict(), dict(device_resident=True, unset_all_valid=True, zero_copy_direct=True)]


@pytest.fixture(scope="module")
def con():
    return da.Connection(0)


def order_key(key):
    """ascending, NULLS LAST; str keys by their UTF-8 bytes"""
    return tuple((1, 0) if k is None else (0, k.encode() if isinstance(k, str) else k) for k in key)


def expected_groups(py, keys, specs, rows):
    """the dict loop: {key tuple: [value per spec]}; float sums as the list of addends"""
    groups = {}
    for r in rows:
        groups.setdefault(tuple(py[k][r] for k in keys), []).append(r)
    out = {}
    for key, members in groups.items():
        vals = []
        for sp in specs:
            op, cols = sp[0], sp[1:]
            if op == "count_star":
                vals.append(len(members))
                continue
            live = [r for r in members if all(py[c][r] is not None for c in cols)]
            if op == "count":
                vals.append(len(live))
            elif not live:
                vals.append(None)
            else:
                v = [py[cols[0]][r] * py[cols[1]][r] if op == "sum_product" else py[cols[0]][r] for r in live]
                if op in ("sum", "sum_product"):
                    vals.append(("fsum", v) if isinstance(v[0], float) else _wrap128(sum(v)))
                else:
                    vals.append((min if op == "min" else max)(v))
        out[key] = vals
    return out


def check_groups(got, want, what):
    assert [g[0] for g in got] == sorted(want, key=order_key), (what, [g[0] for g in got][:6], sorted(want, key=order_key)[:6])
    for key, values in got:
        for g, w in zip(values, want[key]):
            if isinstance(w, tuple):
                exact = math.fsum(w[1])
                bound = 2 * len(w[1]) * 2.0 ** -53 * math.fsum(abs(x) for x in w[1])
                assert abs(g - exact) <= bound, (what, key, g, exact, bound)
            else:
                assert g == w, (what, key, g, w)


def test_the_reference_known_answer_group_by_fruit(con):
    """test/sql/multifile_reading.test: SELECT count(*), fruit FROM read_arrow('data/multifile/glob/*.arrow') GROUP BY fruit -> 3 apple / 3 orange"""
    files = sorted(glob.glob(os.path.join(HERE, "golden", "ref_data", "multifile", "glob", "*.arrow")))
    assert len(files) == 3
    for mode in MODES:
        assert con.read_arrow(files, **mode).group_aggregate(["fruit"], [("count_star",)]) == [(("apple",), [3]), (("orange",), [3])]
    got = con.read_arrow(files).group_aggregate(["fruit"], [("count", "weight"), ("sum", "weight"), ("count", "variety")])
    assert got[0][1][0] == 2 and got[1][1][0] == 2 and got[0][1][2] == 3
    assert abs(got[0][1][1] - (134.2 + 158.6)) < 1e-9 and abs(got[1][1][1] - (142.1 + 96.7)) < 1e-9


Q1_KEYS = ["l_returnflag", "l_linestatus"]
Q1_SPECS = [("sum", "l_quantity"), ("sum", "l_extendedprice"), ("sum_product", "l_extendedprice", "l_discount"), ("sum_product", "l_extendedprice", "l_tax"),
            ("count_star",), ("min", "l_shipdate"), ("max", "l_shipdate"), ("count", "l_comment")]


def _q1_from_pyarrow(table):
    """pyarrow's group_by for what it computes itself; the two products come from the dict loop over the same table"""
    g = table.group_by(Q1_KEYS).aggregate([("l_quantity", "sum"), ("l_extendedprice", "sum"), ([], "count_all"), ("l_shipdate", "min"),
                                           ("l_shipdate", "max"), ("l_comment", "count")]).to_pylist()
    unscaled = lambda d: int(CTX.scaleb(d, 2))
    return {(r["l_returnflag"], r["l_linestatus"]): [unscaled(r["l_quantity_sum"]), unscaled(r["l_extendedprice_sum"]), r["count_all"],
                                                      (r["l_shipdate_min"] - EPOCH).days, (r["l_shipdate_max"] - EPOCH).days, r["l_comment_count"]] for r in g}


def test_q1_shape_on_the_golden_lineitem_against_pyarrow_group_by(con):
    table = ipc.open_stream(LINEITEM).read_all()
    py = _read_back(LINEITEM)
    cutoff = (datetime.date(1998, 9, 2) - EPOCH).days
    assert cutoff == 10471
    for expr in (None, ("l_shipdate", "<=", cutoff)):
        t = table if expr is None else table.filter(pc.less_equal(table["l_shipdate"], pa.scalar(datetime.date(1998, 9, 2))))
        rows = [r for r in range(table.num_rows) if expr is None or py["l_shipdate"][r] <= cutoff]
        want_pa = _q1_from_pyarrow(t)
        want = expected_groups(py, Q1_KEYS, Q1_SPECS, rows)
        if expr is None:      # checked on the CPU: four groups for the 8192 rows
            assert {k: v[2] for k, v in want_pa.items()} == {("N", "O"): 4170, ("R", "F"): 1982, ("A", "F"): 1984, ("N", "F"): 56}
            assert want_pa[("N", "O")][0] == 10691600
        for mode in MODES:
            rel = con.read_arrow(LINEITEM, **mode)
            got, scanned, selected = (rel.filter(expr) if expr else rel).group_aggregate(Q1_KEYS, Q1_SPECS, detail=True)
            assert (scanned, selected) == (table.num_rows, len(rows))
            check_groups(got, want, ("q1", expr, mode))
            assert [g[0] for g in got] == sorted(want_pa)
            for key, v in got:
                assert [v[0], v[1], v[4], v[5], v[6], v[7]] == want_pa[key], (key, v, want_pa[key])


class Fixture:
    pass


@pytest.fixture(scope="module")
def fx(tmp_path_factory):
    rng = np.random.default_rng(777)
    mask = lambda p=0.12: rng.random(N) < p
    arrays = {"k": pa.array(np.arange(N, dtype=np.int64))}
    g = rng.integers(0, 6, N).astype(np.int32)
    g[g == 5] = 4
    g[2 * BATCH_ROWS + 17] = 77                      # a group that first appears in the third record batch ...
    g[: 2 * BATCH_ROWS][g[: 2 * BATCH_ROWS] == 3] = 2  # ... and one more (3) that the first two batches do not have
    m = mask()
    m[2 * BATCH_ROWS + 17] = False
    arrays["g"] = pa.array(g, mask=m)
    arrays["s"] = pa.array([None if x else ("MAIL", "SHIP", "", "REG AIR", "a", "a\0")[i] for i, x in zip(rng.integers(0, 6, N), mask())], pa.string())
    arrays["bin"] = pa.array([None if x else (b"\xff\x00", b"", b"\x00")[i] for i, x in zip(rng.integers(0, 3, N), mask())], pa.binary())
    arrays["date"] = pa.array(rng.integers(9000, 9004, N).astype(np.int32), pa.int32(), mask=mask()).cast(pa.date32())
    hug = [(-1, 0, 1 << 100, -(1 << 100), (1 << 64) + 5)[i] for i in rng.integers(0, 5, N)]
    arrays["hug"] = pa.array([None if x else decimal.Decimal(v) for v, x in zip(hug, mask())], pa.decimal128(38, 0))
    arrays["b"] = pa.array(rng.random(N) < 0.5, mask=mask())
    arrays["u64"] = pa.array(np.array([(1 << 64) - 1, 1 << 63, 5], np.uint64)[rng.integers(0, 3, N)], mask=mask())
    arrays["i64"] = pa.array(rng.integers(-(1 << 62), 1 << 62, N), mask=mask())
    arrays["i32"] = pa.array(rng.integers(-1000, 1000, N).astype(np.int32), mask=mask())
    arrays["f64"] = pa.array(rng.normal(0, 1e4, N) * rng.choice([1e-6, 1.0, 1e6], N), mask=mask())
    arrays["dec"] = pa.array([None if x else CTX.scaleb(decimal.Decimal(int(v)), -2) for v, x in zip(rng.integers(-10 ** 14, 10 ** 14, N), mask())], pa.decimal128(15, 2))
    arrays["c"] = pa.array([None if x else " ".join(("special", "regular", "requests", "bold")[j] for j in rng.integers(0, 4, 3)) for x in mask()], pa.string())
    arrays["f32key"] = pa.array(rng.integers(0, 3, N).astype(np.float32))
    arrays["d"] = pa.array([("x", "y")[i] for i in rng.integers(0, 2, N)], pa.string()).dictionary_encode()
    arrays["lst"] = pa.array([[i % 3] for i in range(N)], pa.list_(pa.int32()))
    arrays["long"] = pa.array([("short", "thirteen bytes")[int(i == N - 5)] for i in range(N)], pa.string())
    table = pa.table(arrays)
    f = Fixture()
    f.path = str(tmp_path_factory.mktemp("groupby") / "t.arrows")
    with ipc.new_stream(f.path, table.schema) as w:
        w.write_table(table, max_chunksize=BATCH_ROWS)
    assert [b.num_rows for b in ipc.open_stream(f.path)] == [4000, 4000, 4000, 3000]
    f.py = _read_back(f.path)
    f.py["b"] = [None if v is None else int(v) for v in f.py["b"]]          # BOOLEAN groups as its byte
    assert 77 not in f.py["g"][: 2 * BATCH_ROWS] and 3 not in f.py["g"][: 2 * BATCH_ROWS] and 3 in f.py["g"]
    return f


SPECS = [("count_star",), ("sum", "i64"), ("min", "hug"), ("max", "dec"), ("sum", "f64"), ("count", "c"), ("sum_product", "i32", "u64"), ("min", "date")]

FILTERS = {
    "none": (None, lambda py, r: True),
    "integer range": (("and", ("i32", ">=", -500), ("i32", "<", 700)), lambda py, r: py["i32"][r] is not None and -500 <= py["i32"][r] < 700),
    "in": (("g", "in", [0, 2, 77]), lambda py, r: py["g"][r] in (0, 2, 77)),
    "string equality": (("s", "=", "SHIP"), lambda py, r: py["s"][r] == "SHIP"),
    "like": (("c", "like", "%special%req%"), lambda py, r: py["c"][r] is not None and "special" in py["c"][r] and "req" in py["c"][r][py["c"][r].index("special") + 7:]),
    "is null": (("dec", "is null"), lambda py, r: py["dec"][r] is None),
}


@pytest.mark.parametrize("name", list(FILTERS))
def test_a_written_table_of_several_batches_under_every_filter_family(con, fx, name):
    expr, keep = FILTERS[name]
    rows = [r for r in range(N) if keep(fx.py, r)]
    assert 0 < len(rows) <= N and (expr is None or len(rows) < N)
    for keys in (["g"], ["s", "date"], ["hug", "b"], ["b", "bin", "u64", "date"]):
        want = expected_groups(fx.py, keys, SPECS, rows)
        if name == "none" and keys == ["g"]:
            assert (77,) in want and (3,) in want and (None,) in want
        results = []
        for mode in MODES[:2]:                       # a device-resident and a host consumer: equal results
            rel = con.read_arrow(fx.path, accept_dictionaries=True, **mode)
            got, scanned, selected = (rel.filter(expr) if expr is not None else rel).group_aggregate(keys, SPECS, detail=True)
            assert (scanned, selected) == (N, len(rows)), (name, keys, mode)
            check_groups(got, want, (name, keys, mode))
            results.append(got)
        assert results[0] == results[1]


def test_a_run_end_encoded_key_column(con, tmp_path):
    rng = np.random.default_rng(8)
    n, per_batch = 9000, 4500
    path = str(tmp_path / "ree.arrows")
    schema = pa.schema([("r", pa.run_end_encoded(pa.int32(), pa.int64())), ("k", pa.int64())])
    with ipc.new_stream(path, schema) as w:
        for first in range(0, n, per_batch):
            ends = np.cumsum(rng.integers(1, 40, 400))
            ends = ends[ends < per_batch].tolist() + [per_batch]
            values = [None if rng.random() < 0.15 else int(v) for v in rng.integers(-3, 3, len(ends))]
            ree = pa.RunEndEncodedArray.from_arrays(pa.array(ends, pa.int32()), pa.array(values, pa.int64()))
            w.write_batch(pa.record_batch([ree, pa.array(np.arange(first, first + per_batch, dtype=np.int64))], schema=schema))
    py = _read_back(path)
    specs = [("count_star",), ("sum", "k"), ("max", "k"), ("count", "r")]
    for expr, rows in ((None, list(range(n))), (("k", ">=", 2500), list(range(2500, n)))):
        for mode in MODES:
            rel = con.read_arrow(path, **mode)
            got = (rel.filter(expr) if expr else rel).group_aggregate(["r"], specs)
            check_groups(got, expected_groups(py, ["r"], specs, rows), ("ree", expr, mode))
            assert got[-1][0] == (None,)


def _merge_by_key(parts, specs):
    """rank lists -> one, merged in the test by key with the rules of SQL"""
    merged = {}
    for part in parts:
        for key, values in part:
            if key not in merged:
                merged[key] = list(values)
                continue
            for i, (sp, v) in enumerate(zip(specs, values)):
                old = merged[key][i]
                if v is None or old is None:
                    merged[key][i] = v if old is None else old
                elif sp[0] in ("min", "max"):
                    merged[key][i] = (min if sp[0] == "min" else max)(old, v)
                else:
                    merged[key][i] = old + v if isinstance(v, float) else (_wrap128(old + v) if sp[0] != "count" and sp[0] != "count_star" else old + v)
    return merged


def test_two_contexts_and_rank_world_merge_to_the_unsharded_result(con, fx):
    keys = ["s", "g"]
    expr = ("i32", "<", 600)
    rows = [r for r in range(N) if fx.py["i32"][r] is not None and fx.py["i32"][r] < 600]
    want = expected_groups(fx.py, keys, SPECS, rows)
    runs = []
    for _ in range(2):
        rel = con.read_arrow(fx.path, accept_dictionaries=True, contexts=[da.Context(0), da.Context(0)], device_resident=True).filter(expr)
        got, scanned, selected = rel.group_aggregate(keys, SPECS, detail=True)
        assert (scanned, selected) == (N, len(rows))
        check_groups(got, want, "two contexts")
        runs.append(got)
    assert runs[0] == runs[1]                        # the two-context double sums are bit-reproducible
    parts = [con.read_arrow(fx.path, accept_dictionaries=True, rank=r, world=2).filter(expr).group_aggregate(keys, SPECS, detail=True) for r in range(2)]
    assert sum(p[1] for p in parts) == N and sum(p[2] for p in parts) == len(rows)
    assert all(0 < len(p[0]) <= len(want) for p in parts)
    merged = _merge_by_key([p[0] for p in parts], SPECS)
    # (a merged double sum is one more addition of two partial sums: n + 1 terms in the bound)
    widened = {k: [("fsum", w[1] + [0.0]) if isinstance(w, tuple) else w for w in v] for k, v in want.items()}
    check_groups(sorted(merged.items(), key=lambda kv: order_key(kv[0])), widened, "rank / world")


def test_refusals_name_the_column_and_a_good_query_follows(con, fx):
    def refused(keys, code, *words, specs=(("count_star",),), expr=None, **options):
        rel = con.read_arrow(fx.path, accept_dictionaries=True, **options)
        try:
            with pytest.raises(da.MiError) as e:
                (rel.filter(expr) if expr else rel).group_aggregate(keys, list(specs))
        finally:
            rel.close()
        assert e.value.code == code, (keys, e.value.code, str(e.value))
        for w in words:
            assert w in str(e.value), (keys, w, str(e.value))

    refused(["f32key"], _ffi.MI_ENOTSUP, "'f32key'", "GROUP BY", "FLOAT")
    refused(["g", "f64"], _ffi.MI_ENOTSUP, "'f64'", "GROUP BY")
    refused(["d"], _ffi.MI_ENOTSUP, "'d'", "GROUP BY", "dictionary")
    refused(["lst"], _ffi.MI_ENOTSUP, "'lst'", "GROUP BY")
    refused(["filename"], _ffi.MI_ENOTSUP, "'filename'", "GROUP BY", "constant", filename=True)
    refused(["nope"], _ffi.MI_EINVAL, "'nope'", "GROUP BY")
    refused(["g", "s", "g"], _ffi.MI_EINVAL, "'g'", "twice")
    refused(["g", "s", "date", "b", "hug"], _ffi.MI_EINVAL, "1 to 4")
    refused(["g"], _ffi.MI_ENOTSUP, "'s'", "SUM", specs=[("sum", "s")])
    # five keys through the C ABI itself
    import ctypes as C
    rel = con.read_arrow(fx.path, accept_dictionaries=True)
    names = (C.c_char_p * 5)(b"g", b"s", b"date", b"b", b"hug")
    spec = (_ffi.AggSpec * 1)()
    spec[0].op = _ffi.AGG_COUNT_STAR
    out_k, out_v, n = (_ffi.GroupKeyValue * 40)(), (_ffi.AggValue * 8)(), C.c_int32(-1)
    assert _ffi.lib().mi_scan_group_aggregate(rel._h, names, 5, spec, 1, out_k, out_v, 8, C.byref(n), None, None) == _ffi.MI_EINVAL
    assert _ffi.lib().mi_scan_group_aggregate(rel._h, names, 0, spec, 1, out_k, out_v, 8, C.byref(n), None, None) == _ffi.MI_EINVAL
    # more groups than the arrays hold: MI_EINVAL with the number found
    assert _ffi.lib().mi_scan_group_aggregate(rel._h, names, 1, spec, 1, out_k, out_v, 2, C.byref(n), None, None) == _ffi.MI_EINVAL
    assert n.value == len({v for v in fx.py["g"]})
    rel.close()
    # a long string in a selected row is refused at run time; deselected, the same query runs
    refused(["long"], _ffi.MI_ENOTSUP, "a VARCHAR / BLOB group key longer than 12 bytes stays above the scan")
    assert con.read_arrow(fx.path, accept_dictionaries=True).filter(("k", "<", N - 5)).group_aggregate(["long"], [("count_star",)]) == [(("short",), [N - 5])]
    # more distinct keys than a window holds
    refused(["k"], _ffi.MI_ENOTSUP, "GROUP BY with more than", "stays above the scan")
    # after init
    rel = con.read_arrow(fx.path, accept_dictionaries=True).project(["k"])
    assert rel.count() == N
    try:
        with pytest.raises(da.MiError) as e:
            rel.group_aggregate(["g"], [("count_star",)])
    finally:
        rel.close()
    assert e.value.code == _ffi.MI_EINVAL and "right after bind" in str(e.value)
    # the same Connection runs a good query, and the ungrouped call still answers
    want = expected_groups(fx.py, ["b"], [("count_star",)], range(N))
    check_groups(con.read_arrow(fx.path, accept_dictionaries=True).group_aggregate(["b"], [("count_star",)]), want, "after the refusals")
    assert con.read_arrow(fx.path, accept_dictionaries=True).aggregate([("count_star",)]) == [N]


def test_a_key_column_absent_from_a_file_is_refused(con, fx, tmp_path):
    other = str(tmp_path / "other.arrows")
    t = pa.table({"k": pa.array(np.arange(10, dtype=np.int64))})
    with ipc.new_stream(other, t.schema) as w:
        w.write_table(t)
    rel = con.read_arrow([fx.path, other], union_by_name=True, accept_dictionaries=True)
    try:
        with pytest.raises(da.MiError) as e:
            rel.group_aggregate(["g"], [("count_star",)])
    finally:
        rel.close()
    assert e.value.code == _ffi.MI_EINVAL and "'g'" in str(e.value) and "absent" in str(e.value)


def test_plain_c_client_prints_the_four_groups_of_q1(tmp_path):
    """examples/q1.c: the predicate through mi_scan_set_filter, keys and aggregates through mi_scan_group_aggregate, from C99"""
    from test_group_aggregate_host import build_q1_example
    exe = build_q1_example(tmp_path)
    r = subprocess.run([exe, LINEITEM], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    py = _read_back(LINEITEM)
    rows = [i for i in range(len(py["l_shipdate"])) if py["l_shipdate"][i] <= 10471]
    want = expected_groups(py, Q1_KEYS, Q1_SPECS, rows)
    lines = r.stdout.splitlines()
    assert lines[0] == "%d groups, %d of %d rows pass" % (len(want), len(rows), len(py["l_shipdate"]))
    body = lines[2:]
    assert len(want) == 4 and len(body) == 4
    for line, key in zip(body, sorted(want)):
        v = want[key]
        dec = lambda x, unit, digits: "%d.%0*d" % (x // unit, digits, x % unit)
        assert line.split() == [key[0], key[1], dec(v[0], 100, 2), dec(v[1], 100, 2), dec(v[2], 10000, 4), dec(v[3], 10000, 4), str(v[4]), str(v[5]),
                                str(v[6]), str(v[7])], (line, key, v)
