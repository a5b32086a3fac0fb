"""Run-end encoded columns (Arrow `+r`) decoded on the MI355X (transcode_run_end, kernels_run_end.hip): every scan entry
point produces the flat vector of the values' type that pyarrow's flattened view holds."""
import os
import struct

import numpy as np
import pyarrow as pa
import pyarrow.compute as pc
import pyarrow.ipc as ipc
import pytest

import duckdb_arrow_amd as da
from duckdb_arrow_amd.hbm import HbmStream

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def con():
    c = da.Connection(0)
    yield c
    c.close()


def make_runs(n, mean_run, seed, null_share=0.1):
    """run ends (int64 numpy) + per-run integer values (None = NULL run) for n rows"""
    rng = np.random.default_rng(seed)
    lens = []
    total = 0
    while total < n:
        k = int(min(n - total, max(1, rng.geometric(1.0 / mean_run))))
        lens.append(k)
        total += k
    ends = np.cumsum(lens).astype(np.int64)
    vals = [None if rng.random() < null_share else int(v) for v in rng.integers(-1000, 1000, len(ends))]
    return ends, vals


def typed_values(vals, typ):
    """python ints (None = NULL) -> an Arrow array of `typ` whose values depend on the ints"""
    def m(f):
        return [None if v is None else f(v) for v in vals]
    if pa.types.is_integer(typ):
        small = typ.bit_width == 8
        unsigned = pa.types.is_unsigned_integer(typ)
        return pa.array(m(lambda v: (v % 100 - (0 if unsigned else 50)) if small else (abs(v) if unsigned else v)), pa.int64()).cast(typ)
    if pa.types.is_float16(typ):
        return pa.array(np.array([0 if v is None else v / 4 for v in vals], np.float16), typ,
                        mask=np.array([v is None for v in vals]))
    if pa.types.is_floating(typ):
        return pa.array(m(lambda v: v / 8), pa.float64()).cast(typ)
    if pa.types.is_boolean(typ):
        return pa.array(m(lambda v: v % 3 == 0), typ)
    if pa.types.is_date32(typ) or pa.types.is_time32(typ):
        return pa.array(m(lambda v: abs(v) * 7), pa.int32()).cast(typ)
    if pa.types.is_date64(typ):
        return pa.array(m(lambda v: (v + 20000) * 86400000), pa.int64()).cast(typ)
    if pa.types.is_time64(typ) or pa.types.is_timestamp(typ) or pa.types.is_duration(typ):
        return pa.array(m(lambda v: abs(v) * 1000003), pa.int64()).cast(typ)
    if typ == pa.month_day_nano_interval():
        return pa.array(m(lambda v: (v % 13, v % 29, v * 1000)), typ)
    if pa.types.is_decimal(typ):
        import decimal
        return pa.array(m(lambda v: decimal.Decimal(v % 100 - 50).scaleb(-1)), typ)
    if pa.types.is_fixed_size_binary(typ):
        return pa.array(m(lambda v: struct.pack("<i", v)[:typ.byte_width].ljust(typ.byte_width, b"z")), typ)
    if typ in (pa.binary(), pa.large_binary(), pa.binary_view()):
        return pa.array(m(lambda v: b"bin%d" % v * (1 + abs(v) % 5)), typ)
    return pa.array(m(lambda v: "value number %d" % v if v % 2 else "v%d" % v), typ)   # utf8 flavours: long and inline


VALUE_TYPES = [pa.int8(), pa.int16(), pa.int32(), pa.int64(), pa.uint8(), pa.uint16(), pa.uint32(), pa.uint64(),
               pa.float16(), pa.float32(), pa.float64(), pa.bool_(), pa.date32(), pa.date64(), pa.time32("s"),
               pa.time32("ms"), pa.time64("us"), pa.time64("ns"), pa.timestamp("us"), pa.timestamp("ns", tz="UTC"),
               pa.timestamp("s", tz="UTC"), pa.duration("s"), pa.duration("ns"), pa.month_day_nano_interval(),
               pa.decimal128(4, 1), pa.decimal128(15, 2), pa.decimal128(38, 10), pa.decimal32(7, 2), pa.decimal64(18, 3),
               pa.decimal64(9, 2), pa.utf8(), pa.large_utf8(), pa.binary(), pa.large_binary(), pa.binary(3),
               pa.string_view(), pa.binary_view()]
RUN_END_TYPES = [pa.int16(), pa.int32(), pa.int64()]


def ree_and_flat(n, mean_run, typ, ret, seed):
    ends, vals = make_runs(n, mean_run, seed)
    if ret == pa.int16() and len(ends) and ends[-1] > 32767:
        raise ValueError("int16 run ends need n <= 32767")
    run_values = typed_values(vals, typ)
    ree = pa.RunEndEncodedArray.from_arrays(pa.array(ends, ret), run_values)
    idx = np.searchsorted(ends, np.arange(n), side="right")
    if pa.types.is_binary_view(typ) or pa.types.is_string_view(typ):   # no take kernel for views
        pv = run_values.to_pylist()
        flat = pa.array([pv[i] for i in idx], typ)
    else:
        flat = run_values.take(pa.array(idx, pa.int64()))
    return ree, flat


def write(path, table, max_chunksize=None, compression=None):
    opts = ipc.IpcWriteOptions(compression=compression) if compression else None
    with ipc.new_stream(path, table.schema, options=opts) as w:
        w.write_table(table, max_chunksize=max_chunksize)
    return path


def same_columns(con, path, names_r, names_p, **kw):
    """scan the run-end encoded columns and their flat twins in one pass: equal python values"""
    rel = con.read_arrow(path, **kw)
    cols = dict(zip(rel.columns, rel.fetch_columns()))
    for r, p in zip(names_r, names_p):
        assert cols[r] == cols[p], (r, kw)
    return cols


@pytest.mark.parametrize("ret", RUN_END_TYPES, ids=str)
def test_every_values_type_equals_the_flat_column(con, tmp_path, ret):
    n = 9000                                  # several 2048-row tiles, runs crossing their boundaries
    cols = {"k": pa.array(np.arange(n), pa.int64())}
    for i, typ in enumerate(VALUE_TYPES):
        r, f = ree_and_flat(n, 5 + 40 * (i % 3), typ, ret, seed=i)
        cols["r%d" % i] = r
        cols["p%d" % i] = f
    t = pa.table(cols)
    path = write(str(tmp_path / "all.arrows"), t, max_chunksize=4000)
    names_r = ["r%d" % i for i in range(len(VALUE_TYPES))]
    names_p = ["p%d" % i for i in range(len(VALUE_TYPES))]
    fields = {f["name"]: f for f in da.Reader(path=path).schema()}
    for r, p in zip(names_r, names_p):
        assert fields[r]["duck_type"] == fields[p]["duck_type"] and fields[r]["kind"] == da._ffi.K_RUN_END
    got = same_columns(con, path, names_r, names_p)
    assert got["k"] == list(range(n))
    # integers against pyarrow's own flattened values
    for i, typ in enumerate(VALUE_TYPES[:8]):
        assert got["r%d" % i] == pc.run_end_decode(t.column("r%d" % i)).to_pylist()
    same_columns(con, path, names_r, names_p, device_resident=True)
    with open(path, "rb") as fh:
        blob = fh.read()
    rel = con.scan_arrow_ipc([np.frombuffer(blob, np.uint8)])
    c2 = dict(zip(rel.columns, rel.fetch_columns()))
    assert all(c2[r] == got[r] for r in names_r)


def test_hbm_resident_equals_the_flat_column(tmp_path):
    n = 20000
    cols = {}
    kinds = [pa.int32(), pa.int64(), pa.decimal128(15, 2), pa.bool_(), pa.float64(), pa.utf8(), pa.timestamp("ns", tz="UTC")]
    for i, typ in enumerate(kinds):
        r, f = ree_and_flat(n, [1, 4, 16, 256, 4096, 3, 50][i], typ, pa.int32(), seed=10 + i)
        cols["r%d" % i], cols["p%d" % i] = r, f
    t = pa.table(cols)
    buf = np.frombuffer(open(write(str(tmp_path / "h.arrows"), t, max_chunksize=7000), "rb").read(), np.uint8).copy()
    ctx = da.Context(0)
    hs = HbmStream(ctx, buf)
    hs.launch()
    assert hs.status() == 0
    hs.launch()                                   # decoded again on every launch
    assert hs.status() == 0
    assert hs.stats()
    for b in hs.fetch():
        by = {c["name"]: c for c in b["columns"]}
        for i in range(len(kinds)):
            r, p = by["r%d" % i], by["p%d" % i]
            assert r["kind"] == da._ffi.K_RUN_END and r["width"] == p["width"]
            nrows, w = b["nrows"], p["width"]
            vr = np.unpackbits(r["validity"].view(np.uint8), bitorder="little")[:nrows].astype(bool)
            vp = np.unpackbits(p["validity"].view(np.uint8), bitorder="little")[:nrows].astype(bool)
            assert np.array_equal(vr, vp), i
            dr = r["data"].reshape(nrows, w)[vp]
            dp = p["data"].reshape(nrows, w)[vp]
            if w == 16 and kinds[i] == pa.utf8():
                dr, dp = dr[:, :8], dp[:, :8]     # length + prefix (long-string pointers point into different heaps)
            assert np.array_equal(dr, dp), i
    hs.close()
    ctx.close()


@pytest.mark.parametrize("case", ["one_run", "unit_runs", "all_null", "empty", "sliced"])
def test_run_shapes(con, tmp_path, case):
    n = 10000
    if case == "one_run":
        r = pa.RunEndEncodedArray.from_arrays(pa.array([n], pa.int32()), pa.array([42], pa.int64()))
        f = pa.array([42] * n, pa.int64())
    elif case == "unit_runs":
        r, f = ree_and_flat(n, 1, pa.int64(), pa.int64(), seed=3)
        r = pa.RunEndEncodedArray.from_arrays(pa.array(np.arange(1, n + 1), pa.int64()), pa.array(np.arange(n) * 3, pa.int64()))
        f = pa.array(np.arange(n) * 3, pa.int64())
    elif case == "all_null":
        r = pa.RunEndEncodedArray.from_arrays(pa.array([100, n], pa.int32()), pa.array([None, None], pa.int64()))
        f = pa.array([None] * n, pa.int64())
    elif case == "empty":
        r = pa.RunEndEncodedArray.from_arrays(pa.array([], pa.int32()), pa.array([], pa.int64()))
        f = pa.array([], pa.int64())
    else:
        r, f = ree_and_flat(n, 30, pa.int64(), pa.int32(), seed=4)
    t = pa.table({"r": r, "p": f})
    if case == "sliced":
        t = t.slice(1234, 6000)
    path = write(str(tmp_path / "s.arrows"), t, max_chunksize=2500)
    for kw in ({}, {"device_resident": True}):
        got = same_columns(con, path, ["r"], ["p"], **kw)
        assert got["r"] == pc.run_end_decode(t.column("r")).to_pylist()


def test_struct_child_with_struct_nulls(con, tmp_path):
    n = 7000
    r, f = ree_and_flat(n, 20, pa.int32(), pa.int32(), seed=5)
    rs, fs = ree_and_flat(n, 9, pa.utf8(), pa.int64(), seed=6)
    mask = pa.array(np.arange(n) % 13 == 0)
    t = pa.table({"st": pa.StructArray.from_arrays([r, rs], names=["x", "y"], mask=mask),
                  "sp": pa.StructArray.from_arrays([f, fs], names=["x", "y"], mask=mask)})
    path = write(str(tmp_path / "st.arrows"), t, max_chunksize=3000)
    for kw in ({}, {"device_resident": True}):
        got = same_columns(con, path, ["st"], ["sp"], **kw)
        assert got["st"] == t.column("sp").to_pylist()


@pytest.mark.parametrize("codec", ["lz4", "zstd"])
def test_compressed_bodies(con, tmp_path, codec):
    n = 12000
    r, f = ree_and_flat(n, 25, pa.int64(), pa.int32(), seed=7)
    rs, fs = ree_and_flat(n, 6, pa.large_utf8(), pa.int64(), seed=8)
    t = pa.table({"r": r, "p": f, "rs": rs, "ps": fs})
    path = write(str(tmp_path / "c.arrows"), t, max_chunksize=5000, compression=codec)
    for kw in ({}, {"device_resident": True}):
        same_columns(con, path, ["r", "rs"], ["p", "ps"], **kw)


def test_from_arrow_and_projection_and_sharding(con, tmp_path):
    n = 16000
    r, f = ree_and_flat(n, 40, pa.int32(), pa.int16(), seed=9)
    t = pa.table({"a": pa.array(np.arange(n), pa.int64()), "r": r, "b": pa.array(np.arange(n) * 2, pa.int64()), "p": f})
    path = write(str(tmp_path / "p.arrows"), t, max_chunksize=3000)
    want = f.to_pylist()
    with open(path, "rb") as fh:
        rel = con.from_arrow(ipc.MessageReader.open_stream(pa.py_buffer(fh.read())))
    assert dict(zip(rel.columns, rel.fetch_columns()))["r"] == want
    assert con.read_arrow(path).project(["b"]).fetch_columns()[0] == list(range(0, 2 * n, 2))
    assert con.read_arrow(path).project(["r", "a"]).fetch_columns()[0] == want
    rows = []
    for rank in range(2):
        a, rr = con.read_arrow(path, rank=rank, world=2).project(["a", "r"]).fetch_columns()
        rows.extend(zip(a, rr))
    assert sorted(rows) == list(zip(range(n), want))


def test_filter_pushdown(con, tmp_path):
    n = 15000
    r, f = ree_and_flat(n, 12, pa.int32(), pa.int32(), seed=11)
    rs, fs = ree_and_flat(n, 7, pa.utf8(), pa.int32(), seed=12)
    t = pa.table({"k": pa.array(np.arange(n), pa.int64()), "r": r, "s": rs})
    path = write(str(tmp_path / "f.arrows"), t, max_chunksize=4000)
    iv, sv = f.to_pylist(), fs.to_pylist()
    cases = [
        (("and", ("r", ">=", -200), ("r", "<=", 300)), lambda i: iv[i] is not None and -200 <= iv[i] <= 300),
        (("r", "in", [5, 17, -3]), lambda i: iv[i] in (5, 17, -3)),
        (("s", "starts_with", "value number 1"), lambda i: sv[i] is not None and sv[i].startswith("value number 1")),
        (("s", "in", ["v12", "v-40", "value number 7"]), lambda i: sv[i] in ("v12", "v-40", "value number 7")),
    ]
    for expr, keep in cases:
        want = [i for i in range(n) if keep(i)]
        for kw in ({}, {"device_resident": True}):
            k, rr, ss = con.read_arrow(path, **kw).filter(expr).fetch_columns()
            assert k == want, expr
            assert rr == [iv[i] for i in want] and ss == [sv[i] for i in want]
    # filter_compact (late materialisation) refuses a run-end encoded column by name
    with pytest.raises(da.MiError) as e:
        con.read_arrow(path, filter_compact=True).filter(("k", "<", 10)).fetch_columns()
    assert e.value.code == da._ffi.MI_ENOTSUP and "'r'" in str(e.value)


def test_copy_writes_the_flat_values_type(con, tmp_path):
    n = 9000
    r, f = ree_and_flat(n, 20, pa.decimal128(15, 2), pa.int32(), seed=13)
    rs, fs = ree_and_flat(n, 5, pa.utf8(), pa.int32(), seed=14)
    t = pa.table({"r": r, "s": rs})
    path = write(str(tmp_path / "src.arrows"), t, max_chunksize=4000)
    out = str(tmp_path / "out.arrows")
    con.copy_to(con.read_arrow(path), out)
    back = ipc.open_stream(out).read_all()
    assert back.column("r").type == pa.decimal128(15, 2) and back.column("s").type == pa.utf8()
    assert back.column("r").to_pylist() == f.to_pylist() and back.column("s").to_pylist() == fs.to_pylist()


def test_damaged_run_ends_are_a_data_error(con, tmp_path):
    # run ends 3, 5, 10 rewritten in the body: not increasing, then ending short of the 10 rows
    t = pa.table({"r": pa.RunEndEncodedArray.from_arrays(pa.array([3, 5, 10], pa.int32()), pa.array([1, 2, 3], pa.int64()))})
    raw = open(write(str(tmp_path / "ok.arrows"), t), "rb").read()
    old = struct.pack("<iii", 3, 5, 10)
    assert raw.count(old) == 1
    for new in (struct.pack("<iii", 5, 3, 10), struct.pack("<iii", 3, 5, 9)):
        path = str(tmp_path / "bad.arrows")
        with open(path, "wb") as fh:
            fh.write(raw.replace(old, new))
        with pytest.raises(da.MiError) as e:
            con.read_arrow(path).fetch_columns()
        assert e.value.code == da._ffi.MI_EINVAL and "run ends" in str(e.value)


def _refused(con, tmp_path, table, name):
    path = write(str(tmp_path / ("%s.arrows" % name)), table)
    with pytest.raises(da.MiError) as e:
        con.read_arrow(path).fetch_columns()
    assert e.value.code == da._ffi.MI_ENOTSUP
    assert name in str(e.value)


def test_refused_inside_lists(con, tmp_path):
    r = pa.RunEndEncodedArray.from_arrays(pa.array([2, 6], pa.int32()), pa.array([1, 2], pa.int64()))
    off = pa.array([0, 2, 6], pa.int32())
    _refused(con, tmp_path, pa.table({"lst": pa.ListArray.from_arrays(off, r)}), "lst")
    _refused(con, tmp_path, pa.table({"big": pa.LargeListArray.from_arrays(pa.array([0, 2, 6], pa.int64()), r)}), "big")
    _refused(con, tmp_path, pa.table({"fix": pa.FixedSizeListArray.from_arrays(r, 3)}), "fix")
    m = pa.MapArray.from_arrays(off, pa.array(["a", "b", "c", "d", "e", "f"]), r)
    _refused(con, tmp_path, pa.table({"mp": m}), "mp")


def test_refused_values(con, tmp_path):
    ends = pa.array([2, 5], pa.int32())
    st = pa.StructArray.from_arrays([pa.array([1, 2])], names=["x"])
    _refused(con, tmp_path, pa.table({"nested": pa.RunEndEncodedArray.from_arrays(ends, st)}), "nested")
    d = pa.array(["x", "y"]).dictionary_encode()
    _refused(con, tmp_path, pa.table({"dict": pa.RunEndEncodedArray.from_arrays(ends, d)}), "dict")
    inner = pa.RunEndEncodedArray.from_arrays(pa.array([1, 2], pa.int32()), pa.array([7, 8], pa.int64()))
    _refused(con, tmp_path, pa.table({"twice": pa.RunEndEncodedArray.from_arrays(ends, inner)}), "twice")


def test_refused_across_files(con, tmp_path):
    d = tmp_path / "mixed"
    d.mkdir()
    write(str(d / "a.arrows"), pa.table({"c": pa.RunEndEncodedArray.from_arrays(pa.array([3], pa.int32()), pa.array([1], pa.int64()))}))
    write(str(d / "b.arrows"), pa.table({"c": pa.array([1, 2, 3], pa.int64())}))
    with pytest.raises(da.MiError) as e:
        con.read_arrow([str(d / "a.arrows"), str(d / "b.arrows")]).fetch_columns()
    assert "c" in str(e.value)
