"""The schema the writer emits for INTERVAL, "NULL" and UNION columns, without a GPU: the Schema message read back by pyarrow
(types, sparse mode, type codes 0 .. m - 1, member names, nullability), FieldFromDuckType(DuckType(f)) for every field of
files the reader binds, the refusals with the column named, and the encode rules of union_format.hpp under ASan + UBSan as a
program of its own (tests/sanitize/union_encode_format_check.cpp).  No sanitizer touches code loaded into Python."""
import os
import shutil
import subprocess

import numpy as np
import pyarrow as pa
import pytest

import duckdb_arrow_amd as da
from duckdb_arrow_amd import _ffi

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EOS = b"\xff\xff\xff\xff\x00\x00\x00\x00"


def _schema(names, types):
    return pa.ipc.read_schema(pa.py_buffer(bytes(da.encode_schema(names, types))))


def _bound(msg):
    r = da.Reader(buffers=[msg + EOS])
    try:
        return [(f["name"], f["duck_type"]) for f in r.schema()]
    finally:
        r.close()


def test_interval_null_and_union_columns_read_back_by_pyarrow():
    names = ["iv", "n", "n2", "u", "s", "w"]
    types = ["INTERVAL", '"NULL"', "null", "UNION(a INTEGER, b VARCHAR)", 'STRUCT(k BIGINT, u UNION(x DOUBLE, "y z" VARCHAR[]))',
             'UNION(s STRUCT(p INTEGER), l INTEGER[], n "NULL", m MAP(VARCHAR, INTEGER), iv INTERVAL)']
    s = _schema(names, types)
    assert s.field("iv").type == pa.month_day_nano_interval() and s.field("n").type == pa.null() and s.field("n2").type == pa.null()
    assert all(s.field(c).nullable for c in names)
    u = s.field("u").type
    assert isinstance(u, pa.SparseUnionType) and u.mode == "sparse" and u.type_codes == [0, 1]
    assert [(u.field(i).name, u.field(i).type, u.field(i).nullable) for i in range(2)] == [("a", pa.int32(), True), ("b", pa.string(), True)]
    su = s.field("s").type.field("u").type
    assert su.mode == "sparse" and su.type_codes == [0, 1]
    assert [(su.field(i).name, su.field(i).type) for i in range(2)] == [("x", pa.float64()), ("y z", pa.list_(pa.field("l", pa.string())))]
    w = s.field("w").type
    assert w.mode == "sparse" and w.type_codes == [0, 1, 2, 3, 4] and [w.field(i).name for i in range(5)] == ["s", "l", "n", "m", "iv"]
    assert w.field(0).type == pa.struct([pa.field("p", pa.int32())]) and w.field(1).type == pa.list_(pa.field("l", pa.int32()))
    assert w.field(2).type == pa.null() and w.field(3).type == pa.map_(pa.string(), pa.int32()) and w.field(4).type == pa.month_day_nano_interval()
    assert all(w.field(i).nullable for i in range(5))
    # ... and the reader of this project binds the message as the types it was made from
    msg = bytes(da.encode_schema(names, types))
    # (the reader prints member names as they are, without the quotes)
    assert _bound(msg) == list(zip(names, ["INTERVAL", '"NULL"', '"NULL"', types[3], types[4].replace('"y z"', "y z"), types[5]]))


def test_32_members_and_one_member():
    many = "UNION(" + ", ".join("m%d %s" % (i, ("INTEGER", "VARCHAR")[i % 2]) for i in range(32)) + ")"
    s = _schema(["u", "one"], [many, "UNION(only BIGINT)"])
    assert s.field("u").type.type_codes == list(range(32)) and s.field("u").type.num_fields == 32
    assert s.field("one").type.type_codes == [0] and s.field("one").type.field(0).name == "only"


def _union_stream():
    n = 6
    ids = pa.array(np.asarray((5, 7), np.int8)[np.arange(n) % 2], pa.int8())
    kids = [pa.array(range(n), pa.int32()), pa.array(["s%d" % r for r in range(n)])]
    dense_kids = [pa.array(range(n), pa.int64()), pa.array([[r] for r in range(n)], pa.list_(pa.int16()))]
    t = pa.table({"us": pa.UnionArray.from_sparse(ids, kids, ["i", "s"], [5, 7]),
                  "ud": pa.UnionArray.from_dense(ids, pa.array(np.arange(n, dtype=np.int32) // 2, pa.int32()), dense_kids, ["a", "b_c"], [5, 7]),
                  "st": pa.StructArray.from_arrays([pa.UnionArray.from_sparse(ids, kids, ["i", "s"], [0, 1]), pa.array(range(n))], ["u", "k"])})
    sink = pa.BufferOutputStream()
    with pa.ipc.new_stream(sink, t.schema) as w:
        w.write_table(t)
    return sink.getvalue().to_pybytes()


def test_every_bound_type_of_the_golden_and_union_files_is_written_back(golden_dir):
    """FieldFromDuckType(DuckType(f)): the duck_type the reader binds, given to the schema writer, is bound as itself again"""
    sources = [open(os.path.join(golden_dir, "edge_types2.arrows"), "rb").read(), _union_stream()]
    seen = set()
    for blob in sources:
        r = da.Reader(buffers=[blob])
        fields = [(f["name"], f["duck_type"]) for f in r.schema()]
        r.close()
        assert fields
        again = _bound(bytes(da.encode_schema([n for n, _ in fields], [t for _, t in fields])))
        assert again == fields
        seen |= {t.split("(")[0] for _, t in fields}
    assert {"INTERVAL", '"NULL"', "UNION", "STRUCT"} <= seen
    # a dense union and type ids 5, 7 come back as a sparse union with the ids 0, 1
    s = _schema(["ud"], ['UNION(a BIGINT, "b c" SMALLINT[])'])
    assert s.field("ud").type.mode == "sparse" and s.field("ud").type.type_codes == [0, 1] and s.field("ud").type.field(1).name == "b c"


@pytest.mark.parametrize("typ, code, text", [
    ("UNION(a INTEGER)[]", _ffi.MI_ENOTSUP, "UNION inside a list"),
    ("UNION(a INTEGER)[3]", _ffi.MI_ENOTSUP, "UNION inside a list"),
    ("STRUCT(x UNION(a INTEGER))[]", _ffi.MI_ENOTSUP, "UNION inside a list"),
    ("MAP(VARCHAR, UNION(a INTEGER))", _ffi.MI_ENOTSUP, "UNION inside a map"),
    ("UNION(a UNION(b INTEGER), c INTEGER)", _ffi.MI_ENOTSUP, "union member 'a' is itself a UNION"),
    ("UNION(" + ", ".join("m%d INTEGER" % i for i in range(33)) + ")", _ffi.MI_ENOTSUP, "more than 32 union members"),
    ("UNION()", _ffi.MI_ENOTSUP, "a union needs at least one member"),
    ("UNION(a INTEGER", _ffi.MI_EINVAL, "malformed type"),
    ("UNION(aINTEGER)", _ffi.MI_EINVAL, "malformed union member"),
    ('UNION("a INTEGER)', _ffi.MI_EINVAL, "malformed union member"),
], ids=lambda v: v[:30] if isinstance(v, str) else str(v))
def test_refusals_name_the_column(typ, code, text):
    with pytest.raises(da.MiError, match=text) as e:
        da.encode_schema(["k", "col"], ["BIGINT", typ])
    assert e.value.code == code and "'col'" in str(e.value)


def test_union_format_encode_rules_alone_under_asan_and_ubsan(tmp_path):
    if shutil.which("g++") is None:
        pytest.skip("no g++")
    exe = str(tmp_path / "union_encode_format_check")
    build = subprocess.run(["g++", "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined",
                            "-I", os.path.join(ROOT, "duckdb-arrow_amd", "csrc"),
                            os.path.join(ROOT, "tests", "sanitize", "union_encode_format_check.cpp"), "-o", exe], capture_output=True, text=True)
    if build.returncode != 0 and "sanitize" in build.stderr.lower() and "cannot find" in build.stderr.lower():
        pytest.skip("sanitizer runtime not installed")
    assert build.returncode == 0, build.stderr[-2000:]
    run = subprocess.run([exe], capture_output=True, text=True, timeout=300, env=dict(os.environ, ASAN_OPTIONS="detect_leaks=1:abort_on_error=0"))
    assert run.returncode == 0, (run.stdout[-1000:], run.stderr[-3000:])
    assert "union_encode_format: ok" in run.stdout


def test_layout_of_union_interval_and_null_nodes_under_asan_and_ubsan(tmp_path):
    """tests/sanitize/writer_types_plan_check.cpp: LayOutBody / EncodeTask / BlocksOfBody / LayOutCompressedBody of union, interval
    and null nodes at 0 to 122 880 rows: one buffer, two, none; a null node first, between, last and as a member."""
    if shutil.which("g++") is None:
        pytest.skip("no g++")
    exe = str(tmp_path / "writer_types_plan_check")
    build = subprocess.run(
        ["g++", "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined", "-I", os.path.join(ROOT, "include"),
         os.path.join(ROOT, "tests", "sanitize", "writer_types_plan_check.cpp"), os.path.join(ROOT, "duckdb-arrow_amd", "csrc", "writer_plan.cpp"),
         "-lpthread", "-o", exe], capture_output=True, text=True)
    if build.returncode != 0 and "sanitize" in build.stderr.lower() and "cannot find" in build.stderr.lower():
        pytest.skip("sanitizer runtime not installed")
    assert build.returncode == 0, build.stderr[-2000:]
    run = subprocess.run([exe], capture_output=True, text=True, timeout=300, env=dict(os.environ, ASAN_OPTIONS="detect_leaks=1:abort_on_error=0"))
    assert run.returncode == 0, (run.stdout[-1000:], run.stderr[-3000:])
    assert " 0 failed" in run.stdout and "FAILED" not in run.stderr, (run.stdout, run.stderr[-3000:])
    assert "Sanitizer" not in run.stderr and "runtime error" not in run.stderr, run.stderr[-3000:]
