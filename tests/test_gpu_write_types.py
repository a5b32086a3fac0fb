"""COPY TO and to_arrow_ipc of UNION, INTERVAL and "NULL" columns, end to end: da.Table -> file / blobs -> pyarrow, the host
scan and the device-resident scan; read -> COPY -> read of files the scan reads (edge_types2.arrows whole, sparse and dense
unions written by pyarrow) through the one-thread sink and the sink-thread pump; file rotation; two sink threads; the
refusals.  The rule this file holds the writer to: every column the scan reads can be written back."""
import os

import numpy as np
import pyarrow as pa
import pyarrow.ipc as ipc
import pytest

import duckdb_arrow_amd as da
from duckdb_arrow_amd import _ffi

import test_gpu_union_scan as us

pytestmark = pytest.mark.gpu

N = 7000
TYPES = {"k": "BIGINT", "iv": "INTERVAL", "nothing": '"NULL"', "u": "UNION(a INTEGER, b VARCHAR)",
         "s": 'STRUCT(k BIGINT, u UNION(x DOUBLE, "yz" VARCHAR[]))',
         "w": 'UNION(s STRUCT(p INTEGER, q VARCHAR), l INTEGER[], n "NULL", m MAP(VARCHAR, INTEGER), iv INTERVAL, big HUGEINT)'}


@pytest.fixture(scope="module")
def con():
    c = da.Connection(0)
    yield c
    c.close()


def _text(i):
    return "t%d" % i if i % 3 else "a string of more than twelve bytes %d" % i


def _rows():
    """-> (what goes into da.Table per column, what every reader must give back per column: bare member values)"""
    put = {c: [] for c in TYPES}
    want = {c: [] for c in TYPES}
    for i in range(N):
        gone = 2040 <= i < 2056 or 4090 <= i < 4100 or i in (63, 64)      # NULL runs over the tile seams and a word seam
        put["k"].append(i)
        iv = None if gone or i % 11 == 0 else (i % 2400 - 1200, 15 - i % 31, (i - 3500) * 123456789)
        put["iv"].append(iv)
        put["nothing"].append(None)
        # u: bare values pick the first member that takes them; a named member may be NULL
        u = None if gone or i % 13 == 0 else (i if i % 2 else _text(i))
        put["u"].append(da.UnionValue("b", None) if u is not None and i % 17 == 0 else u)
        want_u = None if (u is not None and i % 17 == 0) else u
        x = None if i % 7 == 0 else (float(i) / 4 if i % 3 == 0 else [_text(i + j) if j != 1 else None for j in range(i % 4)])
        s = None if gone or i % 19 == 0 else {"k": i * 10**10, "u": x}
        put["s"].append(s)
        pick = i % 8
        w = [None, {"p": i, "q": _text(i)}, [i, None, -i][: i % 4], da.UnionValue("n", None), da.UnionValue("m", {"key%d" % i: i, "other": None}),      # (a bare dict would go to the struct member)
             (1, -i, i * 10**6), da.UnionValue("big", -(1 << 100) + i), {"p": None, "q": None}][pick]
        w = None if gone else w
        put["w"].append(w)
        want_w = w
        if isinstance(w, da.UnionValue):
            want_w = list(w.value.items()) if w.member == "m" else w.value
        want["k"].append(i), want["iv"].append(iv), want["nothing"].append(None), want["u"].append(want_u), want["s"].append(s), want["w"].append(want_w)
    return put, want


@pytest.fixture(scope="module")
def rows():
    return _rows()


def _table(put, names=None):
    names = names or list(TYPES)
    return da.Table(names, [TYPES[c] for c in names], [put[c] for c in names])


def _arrow_python(v):
    """pyarrow's python values -> fetch_columns()'s: intervals as (months, days, micros)"""
    if isinstance(v, pa.MonthDayNano):
        assert v.nanoseconds % 1000 == 0
        return (v.months, v.days, v.nanoseconds // 1000)
    if isinstance(v, dict):
        return {k: _arrow_python(x) for k, x in v.items()}
    if isinstance(v, list):
        return [_arrow_python(x) for x in v]
    if isinstance(v, tuple):
        return tuple(_arrow_python(x) for x in v)
    return v


def _check_arrow(got, want, large=False, views=False):
    got.validate(full=True)
    text = pa.string_view() if views else pa.large_string() if large else pa.string()
    f = got.schema.field
    assert f("iv").type == pa.month_day_nano_interval() and f("nothing").type == pa.null()
    u = f("u").type
    assert u.mode == "sparse" and u.type_codes == [0, 1] and [u.field(i).name for i in range(2)] == ["a", "b"]
    assert u.field(0).type == pa.int32() and u.field(1).type == text and u.field(0).nullable and u.field(1).nullable
    su = f("s").type.field("u").type
    lst = pa.large_list if large else pa.list_
    assert su.mode == "sparse" and su.field(1).name == "yz" and su.field(1).type == lst(pa.field("l", text))
    w = f("w").type
    assert w.type_codes == list(range(6)) and [w.field(i).name for i in range(6)] == ["s", "l", "n", "m", "iv", "big"]
    assert w.field(2).type == pa.null() and w.field(4).type == pa.month_day_nano_interval() and w.field(5).type == pa.decimal128(38, 0)
    for c in TYPES:
        col = got.column(c)
        vals = [_arrow_python(v) for v in col.to_pylist()]
        if c == "w":
            vals = [int(v) if type(v).__name__ == "Decimal" else v for v in vals]
        assert vals == want[c], c
    assert got.column("nothing").null_count == N
    for chunk in got.column("iv").chunks:       # NULL slots are 16 zero bytes
        raw = np.frombuffer(chunk.buffers()[1], np.uint8)[chunk.offset * 16: (chunk.offset + len(chunk)) * 16].reshape(-1, 16)
        assert not raw[~np.array(chunk.is_valid().to_pylist(), bool)].any()
    # no union has a bitmap, and the members' NULL counts are what their bitmaps say
    for chunk in got.column("u").chunks:
        assert chunk.buffers()[0] is None and chunk.null_count == 0
        for k in range(2):
            child = chunk.field(k)
            assert child.null_count == len(child) - sum(child.is_valid().to_pylist())


def _read_back(files):
    return pa.concat_tables([ipc.open_stream(p).read_all() for p in files])


def _nan_safe(v):
    if isinstance(v, float) and v != v:
        return "NaN"
    return [_nan_safe(x) for x in v] if isinstance(v, list) else v


def _columns(rel):
    return dict(zip(rel.columns, [_nan_safe(c) for c in rel.fetch_columns()]))


@pytest.mark.parametrize("options", [{}, {"row_group_size": 2048}, {"row_group_size": 5000}, {"compression": "lz4"}, {"arrow_large_buffer_size": True},
                                     {"produce_arrow_string_view": True}, {"compression": "lz4", "row_group_size": 2048}], ids=str)
def test_copy_to_of_a_table_with_union_interval_and_null_columns(con, rows, tmp_path, options):
    put, want = rows
    files = con.copy_to(_table(put), str(tmp_path / "out.arrows"), **options)
    _check_arrow(_read_back(files), want, options.get("arrow_large_buffer_size", False), options.get("produce_arrow_string_view", False))
    for scan in ({}, {"device_resident": True}):
        rel = con.read_arrow(files, **scan)
        types = dict(zip(rel.columns, rel.types))      # (a HUGEINT leaves as decimal128(38, 0) and is read as that)
        assert types["w"] == TYPES["w"].replace("HUGEINT", "DECIMAL(38,0)") and types["iv"] == "INTERVAL" and types["nothing"] == '"NULL"'
        got = _columns(rel)
        for c in TYPES:
            assert got[c] == want[c], (c, scan)


def test_to_arrow_ipc_of_the_same_table(con, rows):
    put, want = rows
    msgs = con.to_arrow_ipc(_table(put), chunk_size=2048)
    assert msgs[0][1] and not any(h for _, h in msgs[1:]) and len(msgs) == 1 + 4
    got = ipc.open_stream(pa.BufferReader(b"".join(blob for blob, _ in msgs) + b"\xff\xff\xff\xff\x00\x00\x00\x00")).read_all()
    _check_arrow(got, want)


def test_read_copy_read_of_edge_types2_whole(con, golden_dir, tmp_path):
    src = os.path.join(golden_dir, "edge_types2.arrows")
    names = con.read_arrow(src).columns
    assert {"mdn", "dur_s", "dur_ns", "nothing"} <= set(names)
    want = _columns(con.read_arrow(src))
    for i, options in enumerate(({}, {"compression": "lz4"}, {"row_group_size": 2048})):
        files = con.copy_to(con.read_arrow(src), str(tmp_path / ("out%d.arrows" % i)), **options)
        rel = con.read_arrow(files)
        assert rel.columns == names and _columns(rel) == want
        t = _read_back(files)
        t.validate(full=True)
        for c in ("mdn", "dur_s", "dur_ms", "dur_us", "dur_ns"):       # every interval and duration leaves as month_day_nano
            assert t.schema.field(c).type == pa.month_day_nano_interval()
            assert [_arrow_python(v) for v in t.column(c).to_pylist()] == want[c], c
        assert t.schema.field("nothing").type == pa.null() and t.column("nothing").null_count == t.num_rows


def _union_source(tmp_path):
    rng = np.random.default_rng(77)
    batches = []
    for n, first in ((4000, 0), (4100, 4000), (1000, 8100)):
        st = pa.StructArray.from_arrays([us.make_union("sparse", ["int32", "utf8"], (5, 7), n, rng), us.make_union("dense", ["int64", "dec"], (5, 7), n, rng),
                                         pa.array(np.arange(n), pa.int32())], ["a", "b", "k"], mask=pa.array(np.arange(n) % 7 == 3))
        batches.append(pa.record_batch({
            "k": pa.array(first + np.arange(n), pa.int64()), "us": us.make_union("sparse", ["int32", "utf8"], (5, 7), n, rng),
            "ud": us.make_union("dense", ["int64", "utf8"], (5, 7), n, rng),
            "ub": us.make_union("sparse", ["int32", "int64", "dec", "utf8", "list", "struct"], (3, 9, 27, 81, 6, 8), n, rng),
            "dd": us.make_union("dense", ["int32", "int64", "dec", "utf8"], (100, 0, 64, 127), n, rng), "st": st}))
    table = pa.Table.from_batches(batches)
    return us.write(str(tmp_path / "unions.arrows"), table), table


def test_read_copy_read_of_sparse_and_dense_unions_through_both_pumps(con, tmp_path, monkeypatch):
    """the one-thread sink and the sink-thread pump write the same bytes; the fused pump leaves unions to them; a dense union
    comes back sparse, with the type ids 0 .. m - 1 and equal values"""
    src, table = _union_source(tmp_path)
    want = _columns(con.read_arrow(src))
    assert want["ud"] == [us.norm(v) for v in table.column("ud").to_pylist()]
    for rgs, extra in ((4096, {}), (5000, {"compression": "lz4"})):
        outs = []
        for threads in ("1", "4"):
            monkeypatch.setenv("MI_WRITER_THREADS", threads)
            out = str(tmp_path / ("out_%d_%s.arrows" % (rgs, threads)))
            groups0, _ = da.writer_fused_counts()
            con.copy_to(con.read_arrow(src), out, row_group_size=rgs, **extra)
            assert da.writer_fused_counts()[0] == groups0
            outs.append(open(out, "rb").read())
        monkeypatch.delenv("MI_WRITER_THREADS", raising=False)
        assert outs[0] == outs[1]
        got = ipc.open_stream(pa.BufferReader(outs[1])).read_all()
        got.validate(full=True)
        for c in ("us", "ud", "ub", "dd"):
            typ = got.schema.field(c).type
            assert typ.mode == "sparse" and typ.type_codes == list(range(typ.num_fields)), c
            assert [f.name for f in typ] == [f.name for f in table.schema.field(c).type]
            assert [us.norm(v) for v in got.column(c).to_pylist()] == want[c], c
        assert [us.norm(v) for v in got.column("st").to_pylist()] == want["st"]
        for scan in ({}, {"device_resident": True}):
            rel = con.read_arrow(str(tmp_path / ("out_%d_4.arrows" % rgs)), **scan)
            assert rel.types == con.read_arrow(src).types and _columns(rel) == want, scan


def test_file_rotation_with_a_union_column(con, rows, tmp_path):
    put, want = rows
    names = ["k", "u", "iv", "nothing"]
    files = con.copy_to(_table(put, names), str(tmp_path / "rot"), row_group_size=2048, row_groups_per_file=2)
    assert len(files) >= 2
    got = _read_back(files)
    got.validate(full=True)
    assert got.column("u").to_pylist() == want["u"] and got.column("k").to_pylist() == want["k"]
    assert _columns(con.read_arrow(files))["u"] == want["u"]


def test_two_sink_threads_count_nulls_as_their_bitmaps_say(con, rows, tmp_path, monkeypatch):
    """row groups encoded concurrently on two streams: every member's NULL count in the field nodes equals the zero bits of its
    bitmap, in every record batch"""
    put, want = rows
    src = con.copy_to(_table(put, ["k", "u", "w", "iv"]), str(tmp_path / "src.arrows"), row_group_size=3000)
    monkeypatch.setenv("MI_WRITER_THREADS", "2")
    monkeypatch.setenv("MI_WRITER_NO_FUSED", "1")
    out = str(tmp_path / "two.arrows")
    con.copy_to(con.read_arrow(src), out, row_group_size=2048)
    n_batches = 0
    for batch in ipc.open_stream(out):
        n_batches += 1
        for c in ("u", "w"):
            arr = batch.column(c)
            assert arr.null_count == 0
            for k in range(arr.type.num_fields):
                child = arr.field(k)
                if child.type != pa.null():
                    assert child.null_count == len(child) - sum(child.is_valid().to_pylist()), (c, k)
        iv = batch.column("iv")
        assert iv.null_count == len(iv) - sum(iv.is_valid().to_pylist())
    assert n_batches >= 3
    got = _columns(con.read_arrow(out))
    assert got["u"] == want["u"] and got["w"] == want["w"] and got["iv"] == want["iv"]


def test_refusals_at_run_time(con, tmp_path):
    out = str(tmp_path / "no.arrows")
    for typ, text in (("UNION(a INTEGER)[]", "UNION inside a list"), ("UNION(a UNION(b INTEGER))", "is itself a UNION"),
                      ("MAP(VARCHAR, UNION(a INTEGER))", "UNION inside a map"),
                      ("UNION(" + ", ".join("m%d INTEGER" % i for i in range(33)) + ")", "more than 32 union members")):
        with pytest.raises(da.MiError, match=text) as e:
            con.copy_to(da.Table(["col"], [typ], [[None]]), out)
        assert e.value.code == _ffi.MI_ENOTSUP and "'col'" in str(e.value)
        with pytest.raises(da.MiError, match=text):
            con.to_arrow_ipc(da.Table(["col"], [typ], [[None]]))
    # a hand-built vector whose tag names no member under a valid row: the GPU pass reports it, nothing is written for it
    table = da.Table(["u"], ["UNION(a INTEGER, b VARCHAR)"], [[1, "x", 2]])
    keep = []
    chunks = da._chunks_from_table(table, keep)
    import ctypes as C
    C.cast(chunks[0].columns[0].data, C.POINTER(C.c_uint8))[1] = 9
    L = _ffi.lib()
    w = C.c_void_p()
    _ffi.check(L.mi_ipc_serializer_create(con.ctx._h, da._c_fields(table.names, table.types), 1, C.byref(w)))
    try:
        blob, size = C.c_void_p(), C.c_int64()
        arr = (_ffi.DataChunk * 1)(*chunks)
        with pytest.raises(da.MiError, match="Arrow union tag out of range"):
            _ffi.check(L.mi_ipc_serialize_chunks(w, arr, 1, C.byref(blob), C.byref(size)))
    finally:
        L.mi_writer_close(w)
