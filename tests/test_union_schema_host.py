"""Arrow union columns without a GPU: what the host reader binds for pyarrow-written streams (DuckDB type, Arrow C format
string, kind, buffer count), the unions the path refuses as far as the host reader can show it (kind 0 in the schema; the
two refusals the reader itself raises, by code and column name), the Python type parser, the constants of the header and
union_format.hpp under ASan + UBSan as a program of its own (tests/sanitize/union_format_check.cpp).  No sanitizer touches
code loaded into Python."""
import os
import re
import shutil
import struct
import subprocess

import numpy as np
import pyarrow as pa
import pytest

import duckdb_arrow_amd as da
from duckdb_arrow_amd import _ffi

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _stream(table):
    sink = pa.BufferOutputStream()
    with pa.ipc.new_stream(sink, table.schema) as w:
        w.write_table(table)
    return sink.getvalue().to_pybytes()


def _sparse(codes=(5, 7), n=6):
    ids = pa.array(np.asarray(codes, np.int8)[np.arange(n) % 2], pa.int8())
    return pa.UnionArray.from_sparse(ids, [pa.array(range(n), pa.int32()), pa.array(["s%d" % r for r in range(n)])], ["i", "s"], list(codes))


def _dense(codes=(5, 7), n=6):
    ids = pa.array(np.asarray(codes, np.int8)[np.arange(n) % 2], pa.int8())
    offs = pa.array(np.arange(n, dtype=np.int32) // 2, pa.int32())
    return pa.UnionArray.from_dense(ids, offs, [pa.array(range(n), pa.int32()), pa.array(["s%d" % r for r in range(n)])], ["i", "s"], list(codes))


def _schema(table):
    r = da.Reader(buffers=[_stream(table)])
    try:
        return {f["name"]: f for f in r.schema()}
    finally:
        r.close()


def test_schema_of_sparse_and_dense_unions():
    f = _schema(pa.table({"us": _sparse(), "ud": _dense(), "u01": _sparse((0, 1)), "k": pa.array(range(6))}))
    for name, fmt in (("us", "+us:5,7"), ("ud", "+ud:5,7"), ("u01", "+us:0,1")):
        assert f[name]["duck_type"] == "UNION(i INTEGER, s VARCHAR)", f[name]
        assert f[name]["format"] == fmt
        assert f[name]["arrow_type"] == 14 and f[name]["kind"] == _ffi.K_UNION and f[name]["out_width"] == 1 and f[name]["param"] == 2
        # two for the union itself, as always (dense or sparse), plus its members': int32 2, utf8 3
        assert f[name]["n_buffers"] == 2 + 2 + 3
    assert f["us"]["unit"] == 0 and f["ud"]["unit"] == 1
    assert f["k"]["kind"] == _ffi.K_COPY


def test_batch_nodes_of_a_union_carry_type_ids_and_offsets_and_no_validity():
    r = da.Reader(buffers=[_stream(pa.table({"us": _sparse(), "ud": _dense()}))])
    b = r.next_batch()
    nodes = {(n["name"], n["parent"]): n for n in b["nodes"]}
    us, ud = nodes[("us", -1)], nodes[("ud", -1)]
    assert us["kind"] == ud["kind"] == _ffi.K_UNION and us["n_children"] == ud["n_children"] == 2
    assert len(us["spans"]) == 1 and us["spans"][0][1] >= 6          # type ids
    assert len(ud["spans"]) == 2 and ud["spans"][1][1] >= 24         # + int32 offsets
    ids = b["body"][us["spans"][0][0]: us["spans"][0][0] + 6]
    assert ids.tolist() == [5, 7, 5, 7, 5, 7]
    r.close()


def test_nested_members_and_a_union_in_a_struct():
    inner = _sparse((0, 1))
    outer = pa.UnionArray.from_sparse(pa.array([0, 1, 2, 0, 1, 2], pa.int8()),
                                      [pa.array([[1], [2, 3], None, [], [4], [5]], pa.list_(pa.int64())),
                                       pa.StructArray.from_arrays([pa.array(range(6), pa.int16())], ["x"]), inner], ["l", "st", "u"])
    st = pa.StructArray.from_arrays([outer, pa.array(range(6))], ["u", "k"])
    f = _schema(pa.table({"o": outer, "st": st, "n": pa.UnionArray.from_sparse(pa.array([0] * 6, pa.int8()), [pa.nulls(6)], ["z"])}))
    assert f["o"]["duck_type"] == "UNION(l BIGINT[], st STRUCT(x SMALLINT), u UNION(i INTEGER, s VARCHAR))" and f["o"]["kind"] == _ffi.K_UNION
    assert f["o"]["format"] == "+us:0,1,2"
    assert f["st"]["duck_type"] == "STRUCT(u %s, k BIGINT)" % f["o"]["duck_type"] and f["st"]["kind"] == _ffi.K_STRUCT
    assert f["n"]["duck_type"] == 'UNION(z "NULL")' and f["n"]["kind"] == _ffi.K_UNION


def _union_of(members, mode="sparse", n=4):
    ids = pa.array([0] * n, pa.int8())
    names = ["m%d" % k for k in range(len(members))]
    if mode == "sparse":
        return pa.UnionArray.from_sparse(ids, members, names)
    return pa.UnionArray.from_dense(ids, pa.array(range(n), pa.int32()), members, names)


REFUSED = {
    "33_members": lambda: _union_of([pa.array(range(4), pa.int8())] * 33),
    "dictionary_member": lambda: _union_of([pa.array(["a", "b", "a", "b"]).dictionary_encode()]),
    "run_end_member": lambda: _union_of([pa.RunEndEncodedArray.from_arrays(pa.array([2, 4], pa.int32()), pa.array([1, 2], pa.int64()))]),
    "dense_null_member": lambda: _union_of([pa.array(range(4)), pa.nulls(4)], "dense"),
    "dense_list_member": lambda: _union_of([pa.array([[1], [2], [3], [4]], pa.list_(pa.int64()))], "dense"),
    "dense_struct_member": lambda: _union_of([pa.StructArray.from_arrays([pa.array(range(4))], ["x"])], "dense"),
    "dense_union_member": lambda: _union_of([_union_of([pa.array(range(4))])], "dense"),
    "dense_in_sparse": lambda: _union_of([_union_of([pa.array(range(4))], "dense")]),
    "values_of_a_run_end_array": lambda: pa.RunEndEncodedArray.from_arrays(pa.array([1, 4], pa.int32()), _union_of([pa.array(range(2))], n=2)),
}


@pytest.mark.parametrize("name", list(REFUSED))
def test_refused_unions_bind_without_a_kind(name):
    """kind 0 = not decoded on the path: a scan refuses the column at bind with MI_ENOTSUP and its name
    (test_gpu_union_scan.py); the type and the format string are still reported"""
    f = _schema(pa.table({"u": REFUSED[name](), "ok": _union_of([pa.array(range(4))])}))
    assert f["u"]["kind"] == 0 and f["u"]["duck_type"].startswith("UNION(")
    assert (f["u"]["arrow_type"], f["u"]["format"][:2]) in ((14, "+u"), (22, "+r"))
    assert f["ok"]["kind"] == _ffi.K_UNION


def test_32_members_bind():
    f = _schema(pa.table({"u": _union_of([pa.array(range(4), pa.int8())] * 32)}))
    assert f["u"]["kind"] == _ffi.K_UNION and f["u"]["param"] == 32 == _ffi.MAX_UNION_MEMBERS


def _with_metadata_version(stream, version):
    """the stream with Message.version of every message rewritten (V4 = 3, V5 = 4): field 0 of the root table"""
    b = bytearray(stream)
    pos = 0
    while pos + 8 <= len(b):
        cont, mlen = struct.unpack_from("<Ii", b, pos)
        assert cont == 0xFFFFFFFF
        if mlen == 0:
            break
        fb = pos + 8
        table = fb + struct.unpack_from("<I", b, fb)[0]
        vt = table - struct.unpack_from("<i", b, table)[0]
        vt_size = struct.unpack_from("<H", b, vt)[0]
        slot_version = struct.unpack_from("<H", b, vt + 4)[0]
        slot_body = struct.unpack_from("<H", b, vt + 10)[0] if vt_size >= 12 else 0      # bodyLength, absent from a Schema message
        assert slot_version != 0 and struct.unpack_from("<h", b, table + slot_version)[0] == 4
        struct.pack_into("<h", b, table + slot_version, version)
        body = struct.unpack_from("<q", b, table + slot_body)[0] if slot_body else 0
        pos = fb + mlen + body
    return bytes(b)


def test_a_v4_stream_with_a_union_is_refused_by_name_and_others_are_not():
    """V4 unions carry a validity buffer; the buffer walk knows the V5 layout"""
    t = pa.table({"k": pa.array(range(6)), "u": _sparse()})
    v4 = _with_metadata_version(_stream(t), 3)
    r = da.Reader(buffers=[v4])
    with pytest.raises(_ffi.MiError) as e:
        r.next_batch()
    assert e.value.code == _ffi.MI_ENOTSUP and "'u'" in str(e.value) and "V5" in str(e.value)
    r.close()
    r = da.Reader(buffers=[v4])
    r.set_projection(["k"])
    assert r.next_batch()["length"] == 6
    r.close()
    r = da.Reader(buffers=[_stream(t)])
    assert r.next_batch()["length"] == 6
    r.close()


def test_a_big_endian_stream_with_a_union_is_refused_by_name(tmp_path):
    if shutil.which("g++") is None:
        pytest.skip("no g++")
    exe = str(tmp_path / "make_bigendian")
    subprocess.run(["g++", "-std=c++17", "-O1", "-I", os.path.join(ROOT, "include"), os.path.join(ROOT, "tests", "sanitize", "make_bigendian.cpp"),
                    os.path.join(ROOT, "duckdb-arrow_amd", "csrc", "ipc_format.cpp"), "-o", exe], check=True, capture_output=True)
    src, out = str(tmp_path / "le.arrows"), str(tmp_path / "be.arrows")
    with open(src, "wb") as fh:
        fh.write(_stream(pa.table({"k": pa.array(range(6)), "u": _dense()})))
    subprocess.run([exe, src, out], check=True)
    # the tool's schema keeps the union (mode and type ids are re-encoded): pyarrow reads the swapped stream back
    assert pa.ipc.open_stream(open(out, "rb").read()).read_all().column("u").to_pylist() == _dense().to_pylist()
    r = da.Reader(path=out)
    assert {f["name"]: f["format"] for f in r.schema()}["u"] == "+ud:5,7"
    with pytest.raises(_ffi.MiError) as e:
        r.next_batch()
    assert e.value.code == _ffi.MI_ENOTSUP and "'u'" in str(e.value) and "big-endian" in str(e.value)
    r.close()
    r = da.Reader(path=out)
    r.set_projection(["k"])
    assert r.next_batch()["length"] == 6
    r.close()


def test_export_stream_keeps_refusing_unions():
    r = da.Reader(buffers=[_stream(pa.table({"u": _sparse()}))])
    with pytest.raises(Exception) as e:
        r.export_stream().read_all()
    assert "not exported" in str(e.value)


def test_parse_duck_type_knows_unions():
    assert da.parse_duck_type("UNION(i INTEGER, s VARCHAR)") == ("union", [("i", ("leaf", "INTEGER")), ("s", ("leaf", "VARCHAR"))])
    assert da.parse_duck_type('STRUCT(u UNION(a BIGINT[], "b c" STRUCT(x INTEGER)), k BIGINT)') == \
        ("struct", [("u", ("union", [("a", ("list", ("leaf", "BIGINT"))), ("b c", ("struct", [("x", ("leaf", "INTEGER"))]))])), ("k", ("leaf", "BIGINT"))])


def test_header_binding_and_kernel_header_agree():
    raw = open(os.path.join(ROOT, "include", "mi_arrow_ipc.h")).read()
    for text in ("MI_K_UNION = 23", "MI_K_UNION_DENSE = 24", "#define MI_ST_BAD_UNION_TAG 8192u", "#define MI_ST_BAD_UNION_OFFSET 16384u",
                 "#define MI_MAX_UNION_MEMBERS 32"):
        assert text in raw, text
    assert (_ffi.K_UNION, _ffi.K_UNION_DENSE, _ffi.ST_BAD_UNION_TAG, _ffi.ST_BAD_UNION_OFFSET, _ffi.MAX_UNION_MEMBERS) == (23, 24, 8192, 16384, 32)
    hpp = open(os.path.join(ROOT, "duckdb-arrow_amd", "csrc", "union_format.hpp")).read()
    for name, value in (("kMaxMembers", 32), ("kTableEntries", 128), ("kMemberWords", 4)):
        assert re.search(r"constexpr int %s = %d;" % (name, value), hpp), name
    assert _ffi.lib().mi_status_to_error(_ffi.ST_BAD_UNION_TAG) == _ffi.MI_EINVAL
    assert "Arrow union tag out of range" in _ffi.lib().mi_last_error().decode()
    assert _ffi.lib().mi_status_to_error(_ffi.ST_BAD_UNION_OFFSET) == _ffi.MI_EINVAL
    assert _ffi.lib().mi_last_error().decode().startswith("Arrow IPC validation failed: union offsets")


def test_union_format_header_alone_under_asan_and_ubsan(tmp_path):
    if shutil.which("g++") is None:
        pytest.skip("no g++")
    exe = str(tmp_path / "union_format_check")
    build = subprocess.run(["g++", "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined",
                            "-I", os.path.join(ROOT, "duckdb-arrow_amd", "csrc"),
                            os.path.join(ROOT, "tests", "sanitize", "union_format_check.cpp"), "-o", exe], capture_output=True, text=True)
    if build.returncode != 0 and "sanitize" in build.stderr.lower() and "cannot find" in build.stderr.lower():
        pytest.skip("sanitizer runtime not installed")
    assert build.returncode == 0, build.stderr[-2000:]
    run = subprocess.run([exe], capture_output=True, text=True, timeout=300, env=dict(os.environ, ASAN_OPTIONS="detect_leaks=1:abort_on_error=0"))
    assert run.returncode == 0, (run.stdout[-1000:], run.stderr[-3000:])
    assert "union_format: ok" in run.stdout
