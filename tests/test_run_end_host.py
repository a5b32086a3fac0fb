"""Run-end encoded columns (Arrow `+r`) on the host side: schema model, record-batch slicing, projection past such a column,
the Arrow C stream export and the structural checks of damaged metadata.  CPU only."""
import struct

import numpy as np
import pyarrow as pa
import pyarrow.compute as pc
import pyarrow.ipc as ipc
import pytest

import duckdb_arrow_amd as da


def stream_bytes(table, **kw):
    sink = pa.BufferOutputStream()
    with ipc.new_stream(sink, table.schema, **kw) as w:
        w.write_table(table)
    return np.frombuffer(sink.getvalue(), np.uint8).copy()


def ree(values, run_end_type=pa.int32()):
    return pc.run_end_encode(values, run_end_type=run_end_type)


def a_r_b(run_end_type=pa.int32()):
    vals = pa.array([1, 1, 1, None, None, 5, 5, 7, 7, 7], pa.int32())
    return pa.table({"a": pa.array(range(10), pa.int64()), "r": ree(vals, run_end_type),
                     "b": pa.array(range(100, 110), pa.int64())})


def test_schema_reports_run_end_fields():
    t = pa.table({"r": ree(pa.array(["x", "x", None, "y"])), "d": ree(pa.array([1.5, 1.5, 2.0, 2.0]), pa.int64()),
                  "m": ree(pa.array([10, 10, 20, 20], pa.decimal128(15, 2)), pa.int16())})
    fields = da.Reader(buffers=[stream_bytes(t)]).schema()
    assert [f["format"] for f in fields] == ["+r", "+r", "+r"]
    assert [f["duck_type"] for f in fields] == ["VARCHAR", "DOUBLE", "DECIMAL(15,2)"]
    assert [f["arrow_type"] for f in fields] == [22, 22, 22]
    assert all(f["kind"] == da._ffi.K_RUN_END for f in fields)
    assert [f["out_width"] for f in fields] == [16, 8, 8]
    # the field owns no buffers of its own: run_ends owns 2, the values 3 (utf8) or 2
    assert [f["n_buffers"] for f in fields] == [5, 4, 4]


@pytest.mark.parametrize("ret", [pa.int16(), pa.int32(), pa.int64()], ids=str)
def test_spans_match_pyarrow(ret):
    t = a_r_b(ret)
    buf = stream_bytes(t)
    b = da.Reader(buffers=[buf]).next_batch()
    names = [n["name"] for n in b["nodes"]]
    assert names == ["a", "r", "run_ends", "values", "b"]
    rnode = b["nodes"][1]
    assert rnode["spans"] == [] and rnode["n_children"] == 2 and rnode["null_count"] == 0 and rnode["length"] == 10
    # pyarrow's own reader of the same bytes: every buffer at the same place of the body
    rb = ipc.open_stream(pa.py_buffer(buf.tobytes())).read_next_batch()
    base = None
    arrays = [rb.column(0), rb.column(1).run_ends, rb.column(1).values, rb.column(2)]
    nodes = [b["nodes"][i] for i in (0, 2, 3, 4)]
    for arr, nd in zip(arrays, nodes):
        for (off, length), pb in zip(nd["spans"], arr.buffers()):
            if pb is None or length == 0:
                continue
            if base is None:
                base = pb.address - off
            assert pb.address - base == off and pb.size == length
    assert b["nodes"][2]["length"] == 4 and b["nodes"][3]["null_count"] == 1


def test_projection_past_a_run_end_column():
    t = a_r_b()
    for cols in (["b"], ["a", "b"], ["b", "r"]):
        rd = da.Reader(buffers=[stream_bytes(t)])
        rd.set_projection(cols)
        b = rd.next_batch()
        got = da.Reader(buffers=[stream_bytes(t)])
        got.set_projection(cols)
        assert got.export_stream().read_all().equals(t.select(cols))
        assert len(b["column_node"]) == len(cols)
    # the body spans of "b" are those of the full walk
    full = da.Reader(buffers=[stream_bytes(t)]).next_batch()
    rd = da.Reader(buffers=[stream_bytes(t)])
    rd.set_projection(["b"])
    assert rd.next_batch()["nodes"][0]["spans"] == full["nodes"][4]["spans"]


def test_c_stream_export_equals_source():
    n = 5000
    rng = np.random.default_rng(1)
    vals = np.repeat(rng.integers(-50, 50, n // 10), 10)
    t = pa.table({
        "i": ree(pa.array(vals, pa.int64()), pa.int16()),
        "s": ree(pa.array([None if v % 7 == 0 else "run %d" % v for v in vals]), pa.int64()),
        "st": pa.StructArray.from_arrays([ree(pa.array(vals, pa.int32()))], names=["x"],
                                         mask=pa.array(np.arange(n) % 11 == 0)),
        "k": pa.array(np.arange(n), pa.int32()),
    })
    got = da.Reader(buffers=[stream_bytes(t)]).export_stream().read_all()
    got.validate(full=True)
    assert got.equals(t)
    assert got.column("s").combine_chunks().to_pylist() == t.column("s").combine_chunks().to_pylist()


# ---- damaged metadata: the node table of the record batch is patched (FieldNode = {int64 length, int64 null_count})
def _patch_nodes(buf, nodes_before, nodes_after):
    raw = buf.tobytes()
    old = b"".join(struct.pack("<qq", *nd) for nd in nodes_before)
    at = raw.find(old)
    assert at >= 0 and raw.find(old, at + 1) < 0
    new = b"".join(struct.pack("<qq", *nd) for nd in nodes_after)
    return np.frombuffer(raw[:at] + new + raw[at + len(old):], np.uint8).copy()


def _ree_only():
    # r: 10 rows, 4 runs, one NULL value
    return pa.table({"r": ree(pa.array([1, 1, 1, None, None, 5, 5, 7, 7, 7], pa.int32()))})


def _expect_refused(buf, fragment):
    with pytest.raises(da.MiError) as e:
        da.Reader(buffers=[buf]).next_batch()
    assert e.value.code == da._ffi.MI_EINVAL
    assert fragment in str(e.value)
    # the C stream: get_next fails with the same message (pyarrow raises it as OSError), or pyarrow refuses the schema
    with pytest.raises((da.MiError, OSError, pa.ArrowInvalid)):
        da.Reader(buffers=[buf]).export_stream().read_all()


def test_damaged_parent_null_count():
    buf = _patch_nodes(stream_bytes(_ree_only()), [(10, 0), (4, 0), (4, 1)], [(10, 2), (4, 0), (4, 1)])
    _expect_refused(buf, "null_count 2, expected 0")


def test_damaged_run_ends_with_nulls():
    buf = _patch_nodes(stream_bytes(_ree_only()), [(10, 0), (4, 0), (4, 1)], [(10, 0), (4, 1), (4, 1)])
    _expect_refused(buf, "Run ends of column r have null_count 1")


def test_damaged_children_of_different_lengths():
    buf = _patch_nodes(stream_bytes(_ree_only()), [(10, 0), (4, 0), (4, 1)], [(10, 0), (4, 0), (3, 1)])
    _expect_refused(buf, "has 4 run ends but 3 values")


def test_damaged_runs_for_a_non_empty_array():
    buf = _patch_nodes(stream_bytes(_ree_only()), [(10, 0), (4, 0), (4, 1)], [(10, 0), (0, 0), (0, 0)])
    _expect_refused(buf, "of length 10 has 0 runs")


def _u32(b, at):
    return struct.unpack_from("<I", b, at)[0]


def _table_field(b, table, fid):
    """position of field `fid` of a flatbuffer table, or None when absent"""
    vt = table - struct.unpack_from("<i", b, table)[0]
    vt_len = struct.unpack_from("<H", b, vt)[0]
    if 4 + 2 * fid >= vt_len:
        return None
    off = struct.unpack_from("<H", b, vt + 4 + 2 * fid)[0]
    return table + off if off else None


def test_big_endian_stream_with_a_run_end_column_is_refused(tmp_path):
    import os
    import shutil
    import subprocess
    if shutil.which("g++") is None:
        pytest.skip("no g++")
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    tool = str(tmp_path / "make_bigendian")
    subprocess.run(["g++", "-std=c++17", "-O1", "-I", os.path.join(root, "include"), os.path.join(root, "tests", "sanitize", "make_bigendian.cpp"),
                    os.path.join(root, "duckdb-arrow_amd", "csrc", "ipc_format.cpp"), "-o", tool], check=True, capture_output=True)
    t = pa.table({"a": pa.array([1, 2, 3], pa.int64()),
                  "r": pa.RunEndEncodedArray.from_arrays(pa.array([2, 3], pa.int32()), pa.array([7, 8], pa.int64()))})
    # the fixture tool has no layout for run-end encoded bodies: it converts the schema message alone, and the record batch
    # follows as written (the reader refuses the column before it would swap anything)
    le, be = str(tmp_path / "le.arrows"), str(tmp_path / "be.arrows")
    with ipc.new_stream(le, t.schema):
        pass
    subprocess.run([tool, le, be], check=True, capture_output=True)
    schema_le = open(le, "rb").read()[:-8]
    schema_be = open(be, "rb").read()[:-8]
    full = stream_bytes(t).tobytes()
    assert full.startswith(schema_le)
    buf = np.frombuffer(schema_be + full[len(schema_le):], np.uint8).copy()
    with pytest.raises(da.MiError) as e:
        da.Reader(buffers=[buf]).next_batch()
    assert e.value.code == da._ffi.MI_ENOTSUP and "'r'" in str(e.value) and "big-endian" in str(e.value)


def test_damaged_child_count():
    # a struct of three int32 children whose Field.type tag is rewritten to RunEndEncoded (22): three children, not two
    t = pa.table({"r": pa.StructArray.from_arrays([pa.array([3], pa.int32()), pa.array([1], pa.int32()),
                                                   pa.array([2], pa.int32())], names=["run_ends", "values", "x"])})
    raw = bytearray(stream_bytes(t).tobytes())
    meta = 8  # continuation token + length, then the Schema message flatbuffer
    msg = meta + _u32(raw, meta)
    schema_at = _table_field(raw, msg, 2)
    schema = schema_at + _u32(raw, schema_at)
    fields_at = _table_field(raw, schema, 1)
    fields = fields_at + _u32(raw, fields_at)
    field0_at = fields + 4
    field0 = field0_at + _u32(raw, field0_at)
    tag = _table_field(raw, field0, 2)
    assert raw[tag] == 13   # Struct_
    raw[tag] = 22
    buf = np.frombuffer(bytes(raw), np.uint8).copy()
    f = da.Reader(buffers=[buf]).schema()[0]
    assert f["format"] == "+r" and f["kind"] == 0   # not decodable: planned as nothing
    _expect_refused(buf, "has 3 children, expected 2")
